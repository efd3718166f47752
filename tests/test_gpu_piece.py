"""Pieces of several instruments on the device (dusp_score_rows_device, dusp_render_host_score_parts): voices that each lie in a buffer of
their own, of any length and any program, mixed at per-voice onsets in Sum.many's chain order — bit for bit the numpy statement of the
contract (dusp_amd/mix.py score_chain_rows).  The kernel tests feed seeded tensors, ONE ALLOCATION PER VOICE, and need no render; the
render tests hold render_piece to score_chain_rows over the SAME programs' own render(), whatever the tiles."""
import functools

import numpy as np
import pytest

import dusp_amd as d
import score_voices as sv
from conftest import knob_context
from dusp_amd import descriptor, render, runtime, wav
from dusp_amd.mix import score_chain_rows
from test_piece_host import NV_SAW, PLANTED, bits, interleaved_voice

pytestmark = pytest.mark.gpu

GUARD = 64  # floats in front of and behind the output
SENTINEL = np.float32(-12345.678)
ROW_LENGTHS = [1, 3, 254, 257, 773]
# (voices, channels, timeline samples): one sample of everything; 9 and 37 voices (no multiples of the kernel's depth of 8); one and two
# channels; timelines of several workgroups at three residues mod 4
CASES = [(1, 1, 1), (9, 2, 1023), (37, 1, 2317), (37, 2, 1022)]
VARIANTS = ["plain", "gains", "init", "in_place"]
FORMS = {"block256": {}, "doubled_blocks": {"DUSP_SCORE_PLAN_KB": 1}}


def score_context(form):
    return knob_context(48000, **FORMS[form]) if FORMS[form] else render.context(48000)


@functools.lru_cache(maxsize=None)
def batch(case):
    """-> rows (a list, one array [channels, samples_k] per voice), offsets (floats past a 16-byte boundary each row sits at), onsets,
    lengths, gains, init.  Seeded rows of 1, 3, 254, 257 and 773 samples in one list (scales spanning 1e-3 .. 1e3, the planted signed
    zeros, infinities, largest f32, subnormals and a NaN), onsets of both signs and every residue mod 4 — in front of the timeline, next
    to block boundaries, straddling its end, past it, at +-2^62 — and lengths that include 0, 1 and the whole row."""
    n, n_ch, nt = case
    rng = np.random.RandomState(n * 100003 + n_ch * 1009 + nt)
    samples = [ROW_LENGTHS[(k + rng.randint(0, 5)) % 5] for k in range(n)]
    if n == 1:
        samples = [1]
    rows = [(rng.standard_normal((n_ch, s)) * 10.0 ** (k % 7 - 3)).astype(np.float32) for k, s in enumerate(samples)]
    big = [k for k, s in enumerate(samples) if s >= 254]
    for j, v in enumerate(PLANTED if big else []):
        rows[big[j % len(big)]][j % n_ch, 5 + j] = v
    for k in big:
        rows[k][:, 3] = -0.0
    onsets = np.array([rng.randint(-s, nt + 2) for s in samples], dtype=np.int64)
    lengths = np.array([rng.randint(0, s + 1) for s in samples], dtype=np.int64)
    for k in range(n):
        kind = k % 9
        if kind == 1:
            onsets[k] = 256 * rng.randint(0, max(1, nt // 256) + 1) - (k % 4)  # next to a block boundary
        elif kind == 2 and samples[k] <= 256:
            onsets[k], lengths[k] = 256 * rng.randint(0, max(1, nt // 256)) + 256 - samples[k], samples[k]  # the span ends ON a block boundary
        elif kind == 3:
            lengths[k] = samples[k]
        elif kind == 4:
            lengths[k] = 1
        elif kind == 5:
            lengths[k] = 0
        elif kind == 6:
            onsets[k] = (1 << 62) * (1 if k % 2 else -1)
    if n > 2:
        onsets[0], lengths[0] = nt - min(samples[0], 3), samples[0]  # straddles the end
    if n == 1:
        onsets[0], lengths[0] = 0, 1
    offsets = [int(rng.randint(0, 4)) for _ in range(n)]
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
    for a in rows + [onsets, lengths, gains, init]:
        a.setflags(write=False)
    return rows, offsets, onsets, lengths, gains, init


@functools.lru_cache(maxsize=None)
def expected(case, with_lengths, with_gains, with_init, raw):
    rows, _, onsets, lengths, gains, init = batch(case)
    want = score_chain_rows(rows, onsets, case[2], lengths if with_lengths else None, gains if with_gains else None, init if with_init else None, raw)
    want.setflags(write=False)
    return want


def same(got, want, what):
    """bit patterns; for NaN, the positions"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    assert np.array_equal(g, w), "%s: first differing sample %d of %d" % (what, int(np.argmax(g != w)), g.size)


@functools.lru_cache(maxsize=None)
def device_rows(case):
    """every voice's row in an allocation of its own, some 4, 8 or 12 bytes past a 16-byte boundary -> (tensors kept alive, pointers)"""
    import torch
    rows, offsets, *_ = batch(case)
    tensors, pointers = [], []
    for r, off in zip(rows, offsets):
        t = torch.zeros(off + r.size, dtype=torch.float32, device="cuda")
        t[off:] = torch.from_numpy(np.array(r).reshape(-1)).cuda()
        tensors.append(t)
        pointers.append(t.data_ptr() + 4 * off)
    assert len({p % 16 for p in pointers}) > 1 or len(rows) == 1
    return tensors, pointers


def run_rows(ctx, case, with_lengths=True, with_gains=False, init=None, raw=False, out_offset=0):
    """init: None | "buffer" | "in_place".  out_offset: floats past a 16-byte boundary."""
    import torch
    rows, offsets, onsets, lengths, gains, init_host = batch(case)
    n, n_ch, nt = case
    row = n_ch * nt
    tensors, pointers = device_rows(case)
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
    ctx.score_rows_device(pointers, [r.shape[1] for r in rows], n_ch, onsets, nt, d_out.data_ptr() + 4 * lo, lengths if with_lengths else None,
                          d_gains.data_ptr() if with_gains else None, p_init, raw, stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    what = (case, with_lengths, with_gains, init, raw, out_offset)
    assert np.array_equal(out[:lo].view(np.uint32), np.full(lo, SENTINEL).view(np.uint32)), "floats in front of the output were written: %r" % (what,)
    assert np.array_equal(out[lo + row:].view(np.uint32), np.full(GUARD, SENTINEL).view(np.uint32)), "floats behind the output were written: %r" % (what,)
    got = out[lo:lo + row].reshape(n_ch, nt)
    same(got, expected(case, with_lengths, with_gains, init is not None, bool(raw)), what)
    return got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s)))
def test_score_rows_device_equals_the_chain(case, variant, form):
    ctx = score_context(form)
    for raw in (0, 1):
        if variant == "plain":
            run_rows(ctx, case, raw=raw)
            run_rows(ctx, case, with_lengths=False, raw=raw, out_offset=1)
        elif variant == "gains":
            run_rows(ctx, case, with_gains=True, raw=raw, out_offset=2)
        elif variant == "init":
            run_rows(ctx, case, with_gains=True, init="buffer", raw=raw)
            run_rows(ctx, case, init="buffer", raw=raw)
        else:
            run_rows(ctx, case, init="in_place", raw=raw)
            run_rows(ctx, case, with_gains=True, init="in_place", raw=raw, out_offset=3)
    rows, _, *_ = batch(case)
    tensors, _ = device_rows(case)
    for t, r, off in zip(tensors, rows, batch(case)[1]):
        assert np.array_equal(t[off:].cpu().numpy().view(np.uint32), r.reshape(-1).view(np.uint32)), "a row was written to"


def test_the_batches_hold_what_they_are_built_to_hold():
    case = (37, 2, 1022)
    rows, offsets, onsets, lengths, gains, init = batch(case)
    assert {r.shape[1] for r in rows} == set(ROW_LENGTHS) and len(set(offsets)) > 1
    raw, cooked = expected(case, True, False, True, True), expected(case, True, False, True, False)
    assert np.isnan(raw).any() and not np.isnan(cooked).any() and np.isinf(cooked).any()
    assert (np.signbit(raw) & (raw == 0)).any() and not (np.signbit(cooked) & (cooked == 0)).any()
    assert (onsets < 0).any() and (onsets >= case[2]).any() and (np.abs(onsets) == 1 << 62).any() and (lengths == 0).any() and (onsets + lengths > case[2]).any()
    assert {int(o) % 4 for o in onsets} == {0, 1, 2, 3}


def test_no_voices_and_a_first_voice_without_a_row():
    import torch
    ctx = render.context(48000)
    stream = torch.cuda.current_stream().cuda_stream
    init = np.array([[1.0, -0.0, np.nan, 0.0, -2.5, np.inf, 1e-45]], dtype=np.float32)
    d_buf = torch.from_numpy(init.reshape(-1).copy()).cuda()
    d_out = torch.full((7,), 9.0, dtype=torch.float32, device="cuda")
    ctx.score_rows_device([], [], 1, [], 7, d_out.data_ptr(), d_init=d_buf.data_ptr(), raw=True, stream=stream)
    torch.cuda.synchronize()
    same(d_out.cpu().numpy().reshape(1, 7), init, "raw: a copy")
    ctx.score_rows_device([], [], 1, [], 7, d_out.data_ptr(), stream=stream)
    kernel, plan, upload = ctx.score_last_ms()  # (dusp_score_last_ms reports the rows call)
    assert 0 < kernel < 1000 and plan == 0 and upload == 0
    assert not d_out.cpu().numpy().view(np.uint32).any()
    # voice 0 has no row at all (NULL, no samples), voice 1 three samples: the padded entries name voice 0, whose record must be readable
    row = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float32, device="cuda")
    ctx.score_rows_device([None, row.data_ptr()], [0, 3], 1, [2, 3], 7, d_out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tolist() == [0, 0, 0, 1, 2, 3, 0]
    kernel, plan, upload = ctx.score_last_ms()
    assert 0 < kernel < 1000 and 0 <= plan < 1000 and 0 <= upload < 1000


def test_score_rows_device_argument_errors_are_messages():
    import torch
    ctx = render.context(48000)
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p, q = buf.data_ptr(), buf.data_ptr() + 8192
    on = [0, 1]
    for call, needle in [
        (lambda: ctx.score_rows_device([p, p], [8, 8], 1, on, 16, None), "NULL"),
        (lambda: ctx.score_rows_device([p, None], [8, 8], 1, on, 16, q), "row of voice 1 is NULL"),
        (lambda: ctx.score_rows_device([p, p + 2], [8, 8], 1, on, 16, q), "row of voice 1 must be 4-byte aligned"),
        (lambda: ctx.score_rows_device([p, p], [8, 8], 65, on, 16, q), "1..64 channels"),
        (lambda: ctx.score_rows_device([p, p], [8, 8], 1, on, 0, q), "samples of timeline"),
        (lambda: ctx.score_rows_device([p, p], [8, 8], 1, on, (1 << 31) + 1, q), "samples of timeline"),
        (lambda: ctx.score_rows_device([p, p], [8, 8], 2, on, (1 << 30) + 1, q), "channels x timeline samples must not exceed 2\\^31"),  # (sizes only: nothing is touched)
        (lambda: ctx.score_rows_device([p, p], [8, (1 << 30) + 1], 2, on, 16, q), "voice 1: channels x row samples must not exceed 2\\^31"),
        (lambda: ctx.score_rows_device([p, p], [8, 8], 1, on, 16, q + 2), "4-byte aligned"),
        (lambda: ctx.score_rows_device([p, p], [8, 8], 1, on, 16, q, d_gains=p + 3), "4-byte aligned"),
        (lambda: ctx.score_rows_device([p, p], [8, 4], 1, on, 16, q, lengths=[8, 5]), "length of voice 1 is 5"),
        (lambda: ctx.score_rows_device([p, p], [8, 4], 1, on, 16, q, lengths=[-1, 4]), "length of voice 0 is -1"),
    ]:
        with pytest.raises(runtime.DuspHipError, match=needle) as e:
            call()
        assert e.value.status == -1
    for call in (lambda: ctx.score_rows_device([p, p], [8, 8], 1, [0, 0.5], 16, q), lambda: ctx.score_rows_device([p, p], [8], 1, on, 16, q),
                 lambda: ctx.score_rows_device([p, p], [8, -1], 1, on, 16, q), lambda: ctx.score_rows_device([p, p], [8, 8], 1, on, 16, q, lengths=[1.5, 2])):
        with pytest.raises(ValueError, match="dusp-hip"):
            call()
    assert not buf.cpu().numpy().any()  # (nothing ran)


# ---- dusp_render_host_score_parts, render_piece -------------------------------------------------------------------------------------

def jit_context():
    return knob_context(sv.SAMPLE_RATE, DUSP_WAVE_JIT=2)


def voice_samples(n):
    return [sv.NV if k % 2 == 0 else NV_SAW for k in range(n)]


@functools.lru_cache(maxsize=None)
def piece(n):
    """the interleaved list grouped into its two parts, their programs on the compiled kernels, and every voice's row as its OWN program's
    render() gives it -> grouped, programs, rows"""
    d.configure(sv.SAMPLE_RATE)
    grouped = render.piece_parts([descriptor.extract(interleaved_voice(k)) for k in range(n)], voice_samples(n))
    ctx = jit_context()
    programs = [ctx.build(uni.words) for uni, _ in grouped.parts]
    per_part = [prog.render(n_voice, uni.n_instances, uni.params) for prog, (uni, n_voice) in zip(programs, grouped.parts)]
    rows = [np.array(per_part[p][i]) for p, i in zip(grouped.part_of, grouped.instance_of)]
    return grouped, programs, rows


def piece_layout(n):
    """sv.layout's onsets and gains; lengths within every voice's OWN samples (some cut into the sound: the chain is over the same rows)"""
    onsets, _, gains = sv.layout(n)
    rs = np.random.RandomState(1000 + n)
    lengths = np.array([rs.randint(s // 2, s + 1) for s in voice_samples(n)], dtype=np.int64)
    lengths[::5] = np.array(voice_samples(n))[::5]
    return onsets, lengths, gains


@pytest.mark.parametrize("n", [2, 13, 37])
def test_render_piece_is_the_chain_over_the_programs_own_renders(n):
    grouped, programs, rows = piece(n)
    assert len(grouped.parts) == min(n, 2) and [r.shape for r in rows] == [(1, s) for s in voice_samples(n)]
    ctx = jit_context()
    parts = [(prog, n_voice, uni.n_instances, uni.params) for prog, (uni, n_voice) in zip(programs, grouped.parts)]
    onsets, lengths, gains = piece_layout(n)
    want, want_g = score_chain_rows(rows, onsets, sv.NT, lengths), score_chain_rows(rows, onsets, sv.NT, None, gains)
    want_lg = score_chain_rows(rows, onsets, sv.NT, lengths, gains)
    # tiles: the default; one voice a tile; 40000 bytes (about eleven voices of 3092 and 4124 bytes: the 37-voice list in four tiles that
    # split the two parts unevenly); 9000 bytes (two or three voices)
    for tile_bytes in (0, 1, 40000, 9000):
        got = ctx.render_score_parts(parts, grouped.part_of, onsets, sv.NT, lengths, None, tile_bytes)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), (tile_bytes, "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0))))
        assert np.array_equal(bits(ctx.render_score_parts(parts, grouped.part_of, onsets, sv.NT, None, gains, tile_bytes)), bits(want_g)), tile_bytes
        assert np.array_equal(bits(ctx.render_score_parts(parts, grouped.part_of, onsets, sv.NT, lengths, gains, tile_bytes)), bits(want_lg)), tile_bytes
    # voices that began before the timeline, and voices behind its end (a part none of whose voices reaches the timeline is not rendered)
    moved = np.array(onsets)
    moved[::3] -= 400
    moved[1::4] += sv.NT
    want_m = score_chain_rows(rows, moved, sv.NT, lengths, gains)
    for tile_bytes in (0, 9000):
        assert np.array_equal(bits(ctx.render_score_parts(parts, grouped.part_of, moved, sv.NT, lengths, gains, tile_bytes)), bits(want_m)), tile_bytes
    # a plain render afterwards is what it was before; unit state is refused right after a piece and there again after a render
    with pytest.raises(runtime.DuspHipError, match="last render was a mix"):
        programs[0].state(0)
    for prog, (uni, n_voice) in zip(programs, grouped.parts):
        again = prog.render(n_voice, uni.n_instances, uni.params)
        for i in range(uni.n_instances):
            k = int(np.flatnonzero((grouped.part_of == programs.index(prog)) & (grouped.instance_of == i))[0])
            assert np.array_equal(bits(again[i]), bits(rows[k])), "a render after a piece differs from the one before it"
    programs[0].state(0)
    # the surface: the caller's voice list, durations in seconds per voice
    rate = sv.SAMPLE_RATE
    durations = [(s + 0.5) / rate for s in voice_samples(n)]
    d.configure(rate)
    out = d.render_piece([interleaved_voice(k) for k in range(n)], onsets, durations, (sv.NT + 0.5) / rate, lengths, gains, tile_bytes=40000)
    assert out.sampleRate == rate and len(out) == 1 and np.array_equal(bits(out[0]), bits(want_lg[0]))


def test_the_tiles_of_37_voices_split_the_parts_unevenly():
    """what tile_bytes = 40000 does to the 37-voice list (the arithmetic the test above relies on, restated)"""
    row_bytes = [4 * s for s in voice_samples(37)]
    starts, used = [0], 0
    for k, b in enumerate(row_bytes):
        if k > starts[-1] and used + b > 40000:
            starts.append(k)
            used = 0
        used += b
    starts.append(37)
    shares = [(sum(1 for k in range(a, b) if k % 2 == 0), sum(1 for k in range(a, b) if k % 2 == 1)) for a, b in zip(starts, starts[1:])]
    assert len(shares) >= 3 and any(x != y for x, y in shares) and len(set(shares)) > 1, shares


def test_one_structure_and_one_duration_is_render_score():
    d.configure(sv.SAMPLE_RATE)
    n = 13
    onsets, lengths, gains = sv.layout(n)
    dur, voice_dur = (sv.NT + 0.5) / sv.SAMPLE_RATE, (sv.NV + 0.5) / sv.SAMPLE_RATE
    voices = lambda: [sv.voice(k) for k in range(n)]
    want = d.render_score(voices(), onsets, voice_dur, dur, lengths, gains, tile_instances=4)
    for tile_bytes in (0, 10000):
        got = d.render_piece(voices(), onsets, voice_dur, dur, lengths, gains, tile_bytes=tile_bytes)
        assert got.sampleRate == want.sampleRate and len(got) == len(want) == 1 and np.array_equal(bits(got[0]), bits(want[0])), tile_bytes
    assert len(d.render_piece(voices(), onsets, voice_dur, 0)) == 0


def test_render_piece_pcm_and_wav_delivery():
    """s16 / s24 frames and the peak of the PIECE: wav.encode_frames over the f32 timeline, for every normalise mode; the file."""
    n = 13
    rate = sv.SAMPLE_RATE
    d.configure(rate)
    onsets, lengths, gains = piece_layout(n)
    durations = [(s + 0.5) / rate for s in voice_samples(n)]
    voices = lambda: [interleaved_voice(k) for k in range(n)]
    dur = (sv.NT + 0.5) / rate
    piece_f32 = np.stack(d.render_piece(voices(), onsets, durations, dur, lengths, gains, tile_bytes=20000))
    peak_want = np.float32(np.abs(piece_f32).max())
    assert peak_want > 1.0  # (normalise = 1 has something to shrink)
    for depth in (16, 24):
        for normalise in (0, 1, 2):
            res = d.render_piece_pcm(voices(), onsets, durations, dur, depth, normalise, lengths, gains, tile_bytes=20000)
            want, want_peak = wav.encode_frames(piece_f32, depth, normalise)
            assert res.data.dtype == want.dtype and res.data.shape == want.shape and res.bitDepth == depth and res.numberOfChannels == 1
            assert np.array_equal(res.data.view(np.uint8), want.view(np.uint8)), (depth, normalise)
            assert np.float32(res.peak).view(np.uint32) == np.float32(want_peak).view(np.uint32) == peak_want.view(np.uint32)
    file = d.render_piece_wav(voices(), onsets, durations, dur, 16, 0, lengths, gains)
    assert file == wav.encode_wav([c for c in piece_f32], rate, 16) and file[:4] == b"RIFF"


def test_render_score_parts_refusals():
    d.configure(sv.SAMPLE_RATE)
    ctx = jit_context()
    grouped, programs, _ = piece(2)
    (a, na), (b, nb) = [(prog, n_voice) for prog, (_, n_voice) in zip(programs, grouped.parts)]
    pa, pb = grouped.parts[0][0].params, grouped.parts[1][0].params
    out = lambda **kw: ctx.render_score_parts(**kw)
    two = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(2)])
    pan = descriptor.unify([descriptor.extract(d.Pan(d.Osc(200 + 7 * k), -0.5 + 0.25 * k)) for k in range(2)])
    wide = ctx.build(pan.words)
    other = runtime.Context(-1, sv.SAMPLE_RATE)
    elsewhere = other.build(two.words)
    resumable = ctx.build(two.words, runtime.ENGINE_AUTO | runtime.ENGINE_RESUMABLE)
    try:
        for call, needle, status in [
            (lambda: out(parts=[(a, na, 1, pa), (a, na, 1, pa)], part_of=[0, 1], onsets=[0, 1], n_total_samples=128), "parts 0 and 1 are the same program", -1),
            (lambda: out(parts=[(a, na, 1, pa), (wide, 64, 2, pan.params)], part_of=[0, 1, 1], onsets=[0, 1, 2], n_total_samples=128), "part 1 has 2 output channels, part 0 has 1", -1),
            (lambda: out(parts=[(a, na, 1, pa), (elsewhere, 64, 2, two.params)], part_of=[0, 1, 1], onsets=[0, 1, 2], n_total_samples=128), "another context", -1),
            (lambda: out(parts=[(a, na, 1, pa), (b, nb, 1, pb)], part_of=[0, 0], onsets=[0, 1], n_total_samples=128), "names part 0 2 times, the part has 1 instances", -1),
            (lambda: out(parts=[(a, na, 1, pa), (b, nb, 1, pb)], part_of=[0, 1], onsets=[0, 1], n_total_samples=128, lengths=[na, nb + 1]), "length of voice 1 is %d" % (nb + 1), -1),
            (lambda: out(parts=[(a, na, 1, pa), (b, nb, 1, pb)], part_of=[0, 1], onsets=[0, 1], n_total_samples=0), "timeline", -1),
            (lambda: out(parts=[(a, na, 1, pa), (b, 0, 1, pb)], part_of=[0, 1], onsets=[0, 1], n_total_samples=128), "n_samples", -1),
            (lambda: out(parts=[(a, na, 1, pa), (resumable, 64, 2, two.params)], part_of=[0, 1, 1], onsets=[0, 1, 2], n_total_samples=128), "resumable", -2),
        ]:
            with pytest.raises(runtime.DuspHipError, match=needle) as e:
                call()
            assert e.value.status == status, needle
        for call, needle in [
            (lambda: out(parts=[(a, na, 1, pa)], part_of=[0, 1], onsets=[0, 1], n_total_samples=128), "part_of names a part"),
            (lambda: out(parts=[(a, na, 1, pa), (b, nb, 1, pb)], part_of=[0, 1], onsets=[0, 0.5], n_total_samples=128), "whole numbers"),
            (lambda: out(parts=[(a, na, 1, pa), (b, nb, 1, pb)], part_of=[0, 1], onsets=[0, 1], n_total_samples=128, gains=[1.0]), "gains must have shape"),
            (lambda: out(parts=[], part_of=[], onsets=[], n_total_samples=128), "at least one part"),
        ]:
            with pytest.raises(ValueError, match=needle):
                call()
        assert out(parts=[(a, na, 1, pa), (b, nb, 1, pb)], part_of=[1, 0], onsets=[5, 0], n_total_samples=128).shape == (1, 128)  # (and it still renders)
    finally:  # (programs before their context, whatever failed)
        for prog in (wide, elsewhere, resumable):
            prog.close()
        other.close()
