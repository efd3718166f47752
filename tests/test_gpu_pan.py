"""Stereo placement on the device (dusp_score_rows_pan_device, dusp_render_host_score_parts_pan): mono voices, each in a buffer of its
own, panned where they are added to a two-channel timeline — bit for bit the numpy statement of the contract (dusp_amd/mix.py
score_chain_rows_panned), and, through render_piece(..., pans=...), bit for bit the oracle's render of the piece as ONE circuit with the
reference's Pan unit behind every voice.  The kernel tests feed the planted rows of tests/pan_cases.py, ONE ALLOCATION PER VOICE, and
need no render."""
import functools

import numpy as np
import pytest

import dusp_amd as d
import score_voices as sv
from conftest import knob_context
from dusp_amd import descriptor, render, runtime, wav
from dusp_amd.mix import score_chain_rows_panned
from pan_cases import as_one_panned_circuit, pans_for, planted
from test_piece_host import NV_SAW, bits, interleaved_voice

pytestmark = pytest.mark.gpu

NT = 1301  # (five workgroups of 256 and 21 samples)
GUARD = 64  # floats in front of and behind the output
SENTINEL = np.float32(-12345.678)
COUNTS = [1, 8, 9, 37]  # a lone voice, one full batch of the kernel's depth, one more, four batches and five
VARIANTS = ["plain", "gains", "init", "in_place"]
FORMS = {"block256": {}, "doubled_blocks": {"DUSP_SCORE_PLAN_KB": 1}}


def pan_context(form):
    return knob_context(48000, **FORMS[form]) if FORMS[form] else render.context(48000)


@functools.lru_cache(maxsize=None)
def expected(n, with_lengths, with_gains, with_init, raw, lo=0, hi=NT):
    """the contract over the window [lo, hi) of the timeline: the same chain with shifted onsets"""
    rows, onsets, lengths, gains, pans, init = planted(n, NT)
    want = score_chain_rows_panned(rows, onsets - lo, pans, hi - lo, lengths if with_lengths else None, gains if with_gains else None,
                                   np.ascontiguousarray(init[:, lo:hi]) if with_init else None, raw)
    want.setflags(write=False)
    return want


def same(got, want, what):
    """bit patterns; for NaN, the positions"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    assert np.array_equal(g, w), "%s: first differing sample %d of %d" % (what, int(np.argmax(g != w)), g.size)


@functools.lru_cache(maxsize=None)
def device_rows(n):
    """every voice's row in an allocation of its own, 0, 4, 8 or 12 bytes past a 16-byte boundary; none at all for a row of no samples"""
    import torch
    rows = planted(n, NT)[0]
    tensors, pointers = [], []
    for k, r in enumerate(rows):
        if r.size == 0:
            tensors.append(None)
            pointers.append(None)
            continue
        off = k % 4
        t = torch.zeros(off + r.size, dtype=torch.float32, device="cuda")
        t[off:] = torch.from_numpy(np.array(r).reshape(-1)).cuda()
        tensors.append(t)
        pointers.append(t.data_ptr() + 4 * off)
    return tensors, pointers


def run_pan(ctx, n, with_lengths=True, with_gains=False, init=None, raw=False, out_offset=0, lo=0, hi=NT):
    """init: None | "buffer" | "in_place".  out_offset: floats past a 16-byte boundary.  [lo, hi): the window of the timeline."""
    import torch
    rows, onsets, lengths, gains, pans, init_host = planted(n, NT)
    nt = hi - lo
    row = 2 * nt
    _, pointers = device_rows(n)
    d_out = torch.full((GUARD + out_offset + row + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    at = GUARD + out_offset
    d_gains = torch.from_numpy(np.array(gains)).cuda() if with_gains else None
    d_init, p_init = None, None
    window = np.ascontiguousarray(init_host[:, lo:hi]).reshape(-1)
    if init == "in_place":
        d_out[at:at + row] = torch.from_numpy(window.copy()).cuda()
        p_init = d_out.data_ptr() + 4 * at
    elif init == "buffer":
        d_init = torch.from_numpy(window.copy()).cuda()
        p_init = d_init.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.score_rows_pan(pointers, [r.shape[1] for r in rows], onsets - lo, pans, nt, d_out.data_ptr() + 4 * at, lengths if with_lengths else None,
                       d_gains.data_ptr() if with_gains else None, p_init, raw, stream=stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    what = (n, with_lengths, with_gains, init, raw, out_offset, lo, hi)
    assert np.array_equal(out[:at].view(np.uint32), np.full(at, SENTINEL).view(np.uint32)), "floats in front of the output were written: %r" % (what,)
    assert np.array_equal(out[at + row:].view(np.uint32), np.full(GUARD, SENTINEL).view(np.uint32)), "floats behind the output were written: %r" % (what,)
    got = out[at:at + row].reshape(2, nt)
    same(got, expected(n, with_lengths, with_gains, init is not None, bool(raw), lo, hi), what)
    return got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", COUNTS)
def test_score_rows_pan_equals_the_panned_chain(n, variant, form):
    ctx = pan_context(form)
    for raw in (0, 1):
        if variant == "plain":
            run_pan(ctx, n, raw=raw)
            run_pan(ctx, n, with_lengths=False, raw=raw, out_offset=1)
        elif variant == "gains":
            run_pan(ctx, n, with_gains=True, raw=raw, out_offset=2)
        elif variant == "init":
            run_pan(ctx, n, with_gains=True, init="buffer", raw=raw)
            run_pan(ctx, n, init="buffer", raw=raw)
        else:
            run_pan(ctx, n, init="in_place", raw=raw)
            run_pan(ctx, n, with_gains=True, init="in_place", raw=raw, out_offset=3)
    tensors, _ = device_rows(n)
    for k, (t, r) in enumerate(zip(tensors, planted(n, NT)[0])):
        assert t is None or np.array_equal(t[k % 4:].cpu().numpy().view(np.uint32), r.reshape(-1).view(np.uint32)), "a row was written to"


@pytest.mark.parametrize("form", list(FORMS))
def test_a_window_of_the_timeline_is_the_same_chain_with_shifted_onsets(form):
    """window edges that are no multiples of 256: the pieces, raw and continued in place, are the whole timeline's bits"""
    ctx = pan_context(form)
    whole = expected(37, True, True, True, True)
    pieces = [run_pan(ctx, 37, with_gains=True, init="in_place", raw=True, out_offset=k % 4, lo=lo, hi=hi) for k, (lo, hi) in enumerate([(0, 300), (300, 1001), (1001, NT)])]
    same(np.concatenate(pieces, axis=1), whole, "windows")
    run_pan(ctx, 9, init="buffer", lo=13, hi=899)


def test_the_chain_cut_into_two_launches_and_continued_raw_is_the_whole():
    """voices [0, 20) raw, then [20, 37) in place through init: what the tiles of a piece do"""
    import torch
    ctx = pan_context("block256")
    rows, onsets, lengths, gains, pans, _ = planted(37, NT)
    _, pointers = device_rows(37)
    samples = [r.shape[1] for r in rows]
    d_out = torch.zeros(2 * NT, dtype=torch.float32, device="cuda")
    d_gains = torch.from_numpy(np.array(gains)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.score_rows_pan(pointers[:20], samples[:20], onsets[:20], pans[:20], NT, d_out.data_ptr(), lengths[:20], d_gains.data_ptr(), None, True, stream=stream)
    ctx.score_rows_pan(pointers[20:], samples[20:], onsets[20:], pans[20:], NT, d_out.data_ptr(), lengths[20:], d_gains.data_ptr() + 4 * 20, d_out.data_ptr(), False, stream=stream)
    torch.cuda.synchronize()
    kernel, plan, upload = ctx.score_last_ms()  # (dusp_score_last_ms reports the panned call)
    assert 0 < kernel < 1000 and 0 <= plan < 1000 and 0 < upload < 1000
    same(d_out.cpu().numpy().reshape(2, NT), expected(37, True, True, False, False), "two launches")


def test_no_voices_a_first_voice_without_a_row_and_a_given_compensation():
    import torch
    ctx = render.context(48000)
    stream = torch.cuda.current_stream().cuda_stream
    init = np.array([[1.0, -0.0, np.nan, 0.0, -2.5, np.inf, 1e-45], [-0.0, 3.0, 0.0, np.nan, -np.inf, 2.0, -1e-45]], dtype=np.float32)
    d_buf = torch.from_numpy(init.reshape(-1).copy()).cuda()
    d_out = torch.full((14,), 9.0, dtype=torch.float32, device="cuda")
    ctx.score_rows_pan([], [], [], [], 7, d_out.data_ptr(), d_init=d_buf.data_ptr(), raw=True, stream=stream)
    torch.cuda.synchronize()
    same(d_out.cpu().numpy().reshape(2, 7), init, "raw: a copy of both channels")
    ctx.score_rows_pan([], [], [], [], 7, d_out.data_ptr(), d_init=d_buf.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    same(d_out.cpu().numpy().reshape(2, 7), score_chain_rows_panned([], [], [], 7, init=init), "`|| 0` of both channels")
    # voice 0 has no row at all (NULL, no samples), voice 1 three samples: the padded entries name voice 0, whose record must be readable
    row = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float32, device="cuda")
    ctx.score_rows_pan([None, row.data_ptr()], [0, 3], [2, 3], [0.5, -1.0], 7, d_out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tolist() == [0, 0, 0, 1, 2, 3, 0] + [0] * 7
    # pan 0 with a compensation of 2: the mono sample on both channels
    ctx.score_rows_pan([row.data_ptr()], [3], [1], [0.0], 7, d_out.data_ptr(), comp=[2.0], stream=stream)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tolist() == [0, 1, 2, 3, 0, 0, 0] * 2


# ---- dusp_render_host_score_parts_pan, render_piece(..., pans=...) -------------------------------------------------------------------------

def voice_samples(n):
    return [sv.NV if k % 2 == 0 else NV_SAW for k in range(n)]


def piece_args(n):
    rate = sv.SAMPLE_RATE
    onsets, _, gains = sv.layout(n)
    return onsets, gains, pans_for(n), [(s + 0.5) / rate for s in voice_samples(n)], (sv.NT + 0.5) / rate


@functools.lru_cache(maxsize=None)
def oracle_piece(n, with_gains, oracle):
    """the oracle's render of the panned piece as ONE circuit (tests/test_pan_host.py anchors the numpy contract to it)"""
    d.configure(sv.SAMPLE_RATE)
    onsets, gains, pans, _, _ = piece_args(n)
    circuit = as_one_panned_circuit([interleaved_voice(k) for k in range(n)], onsets, pans, gains if with_gains else None)
    want = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("n", [2, 13, 37])
def test_render_piece_with_pans_is_the_oracles_one_circuit(n, with_gains, oracle):
    want = oracle_piece(n, with_gains, oracle)
    assert want.shape == (2, sv.NT)
    onsets, gains, pans, durations, dur = piece_args(n)
    g = gains if with_gains else None
    d.configure(sv.SAMPLE_RATE)
    voices = lambda: [interleaved_voice(k) for k in range(n)]
    # tiles: the default (one), and 9000 bytes — two voices of 3092 and 4124 bytes a tile: seven tiles for 13 voices, nineteen for 37 (two voices: a tile each)
    results = {}
    for tile_bytes in (0, 9000) if n > 2 else (0, 1):
        got = d.render_piece(voices(), onsets, durations, dur, None, g, tile_bytes=tile_bytes, pans=pans)
        assert got.sampleRate == sv.SAMPLE_RATE and len(got) == 2 and got[0].shape == (sv.NT,)
        results[tile_bytes] = np.stack(got)
    a, b = results.values()
    print("n %d gains %s: %d samples differ between the tilings, %d from the oracle" % (n, with_gains, int((bits(a) != bits(b)).sum()), int((bits(a) != bits(want)).sum())))
    assert np.array_equal(bits(a), bits(b)), "the two tilings differ"
    for tile_bytes, got in results.items():
        assert np.array_equal(bits(got), bits(want)), (tile_bytes, "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0))))


def test_the_small_tile_cuts_the_voice_lists_into_at_least_three_tiles():
    """what tile_bytes = 9000 does to mono rows of 3092 and 4124 bytes in turn (the arithmetic the test above relies on, restated)"""
    for n, least in ((13, 3), (37, 3)):
        row_bytes = [4 * s for s in voice_samples(n)]
        starts, used = [0], 0
        for k, b in enumerate(row_bytes):
            if k > starts[-1] and used + b > 9000:
                starts.append(k)
                used = 0
            used += b
        assert len(starts) >= least, (n, starts)


def test_render_score_with_pans_is_render_piece_of_one_structure(oracle):
    d.configure(sv.SAMPLE_RATE)
    n = 13
    onsets, lengths, gains = sv.layout(n)
    pans = pans_for(n)
    dur, voice_dur = (sv.NT + 0.5) / sv.SAMPLE_RATE, (sv.NV + 0.5) / sv.SAMPLE_RATE
    voices = lambda: [sv.voice(k) for k in range(n)]
    want = d.render_piece(voices(), onsets, voice_dur, dur, lengths, gains, pans=pans)
    got = d.render_score(voices(), onsets, voice_dur, dur, lengths, gains, pans=pans)
    assert got.sampleRate == want.sampleRate and len(got) == len(want) == 2
    assert np.array_equal(bits(np.stack(got)), bits(np.stack(want))) and np.abs(np.stack(got)).max() > 0
    # ... and, lengths only cutting off zeros, the oracle's one circuit of the score voices
    circuit = as_one_panned_circuit(voices(), onsets, pans, gains)
    ref = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
    assert np.array_equal(bits(np.stack(got)), bits(ref))
    assert len(d.render_score(voices(), onsets, voice_dur, 0, pans=pans)) == 0
    # without pans nothing has changed: one channel
    assert len(d.render_score(voices(), onsets, voice_dur, dur, lengths, gains)) == 1


def test_render_piece_pcm_and_wav_with_pans():
    """s16 / s24 / f32 frames and the peak of the panned piece: wav.encode_frames over the f32 result, two channels a frame; the file."""
    n = 13
    rate = sv.SAMPLE_RATE
    d.configure(rate)
    onsets, gains, pans, durations, dur = piece_args(n)
    voices = lambda: [interleaved_voice(k) for k in range(n)]
    piece_f32 = np.stack(d.render_piece(voices(), onsets, durations, dur, None, gains, tile_bytes=20000, pans=pans))
    peak_want = np.float32(np.abs(piece_f32).max())
    assert piece_f32.shape == (2, sv.NT) and peak_want > 1.0  # (normalise = 1 has something to shrink)
    for depth, normalise in ((16, 0), (16, 1), (24, 2), (32, 0)):
        res = d.render_piece_pcm(voices(), onsets, durations, dur, depth, normalise, None, gains, tile_bytes=20000, pans=pans)
        want, want_peak = wav.encode_frames(piece_f32, depth, normalise)
        assert res.data.dtype == want.dtype and res.data.shape == want.shape and res.bitDepth == depth and res.numberOfChannels == 2
        assert np.array_equal(res.data.view(np.uint8), want.view(np.uint8)), (depth, normalise)
        assert np.float32(res.peak).view(np.uint32) == np.float32(want_peak).view(np.uint32) == peak_want.view(np.uint32)
    file = d.render_piece_wav(voices(), onsets, durations, dur, 16, 0, None, gains, pans=pans)
    assert file == wav.encode_wav([c for c in piece_f32], rate, 16) and file[:4] == b"RIFF"
    score_file = d.render_score_wav([sv.voice(k) for k in range(3)], [0, 10, 20], durations[0], dur, 16, 0, pans=[-1, 0, 1])
    score_f32 = np.stack(d.render_score([sv.voice(k) for k in range(3)], [0, 10, 20], durations[0], dur, pans=[-1, 0, 1]))
    assert score_file == wav.encode_wav([c for c in score_f32], rate, 16)


def test_refusals_on_a_live_context():
    import ctypes
    import torch
    d.configure(sv.SAMPLE_RATE)
    ctx = knob_context(sv.SAMPLE_RATE, DUSP_WAVE_JIT=2)
    mono = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(2)])
    wide_uni = descriptor.unify([descriptor.extract(d.Pan(d.Osc(200 + 7 * k), -0.5 + 0.25 * k)) for k in range(2)])
    a, wide = ctx.build(mono.words), ctx.build(wide_uni.words)
    try:
        with pytest.raises(runtime.DuspHipError, match="dusp_render_host_score_parts_pan: part 1 has 2 output channels: a panned voice is mono") as e:
            ctx.render_score_parts([(a, 64, 2, mono.params), (wide, 64, 2, wide_uni.params)], [0, 1, 0, 1], [0, 1, 2, 3], 128, pans=[0, 0, 0, 0])
        assert e.value.status == -1
        with pytest.raises(runtime.DuspHipError, match="part 0 has 2 output channels: a panned voice is mono"):
            ctx.render_score_parts([(wide, 64, 2, wide_uni.params)], [0, 0], [0, 1], 128, pans=[0, 0])
        for pans in ([0, float("nan")], [float("inf"), 0]):
            with pytest.raises(ValueError, match="dusp-hip: the pan of voice %d is not finite" % (1 if pans[0] == 0 else 0)):
                ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, pans=pans)
        with pytest.raises(ValueError, match="pans must have shape"):
            ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, pans=[0])
        # the library's own check, behind the binder's: a NaN pan handed to the C call
        buf = torch.zeros(1024, dtype=torch.float32, device="cuda")
        rows = np.array([buf.data_ptr(), buf.data_ptr()], dtype=np.uint64)
        samples, onsets = np.array([8, 8], dtype=np.uint32), np.array([0, 1], dtype=np.int64)
        bad = np.array([0.0, np.nan], dtype=np.float32)
        rc = ctx._L.dusp_score_rows_pan_device(ctx._h, rows.ctypes.data, samples.ctypes.data, 2, onsets.ctypes.data, None, None, bad.ctypes.data, None, 16, None, 0,
                                               buf.data_ptr() + 2048, None)
        assert rc == -1 and b"dusp_score_rows_pan_device: the pan of voice 1 is not finite" in ctx._L.dusp_last_error(ctx._h)
        table = (runtime.ScorePart * 1)(runtime.ScorePart(a._h, 2, 64, mono.params.ctypes.data if mono.params is not None else None))
        part_of, out = np.zeros(2, dtype=np.uint32), np.zeros((2, 128), dtype=np.float32)
        rc = ctx._L.dusp_render_host_score_parts_pan(table, 1, 2, part_of.ctypes.data, onsets.ctypes.data, None, None, bad.ctypes.data, None, 128, 0, 0, 0, out.ctypes.data, None)
        assert rc == -1 and b"dusp_render_host_score_parts_pan: the pan of voice 1 is not finite" in ctx._L.dusp_last_error(ctx._h)
        for call, needle in [
            (lambda: ctx.score_rows_pan([buf.data_ptr()] * 2, [8, 8], [0, 1], [0, 0], (1 << 30) + 1, buf.data_ptr() + 2048), "channels x timeline samples must not exceed 2\\^31"),
            (lambda: ctx.score_rows_pan([buf.data_ptr(), None], [8, 8], [0, 1], [0, 0], 16, buf.data_ptr() + 2048), "dusp_score_rows_pan_device: the row of voice 1 is NULL"),
            (lambda: ctx.score_rows_pan([buf.data_ptr()] * 2, [8, 4], [0, 1], [0, 0], 16, buf.data_ptr() + 2048, lengths=[8, 5]), "length of voice 1 is 5"),
            (lambda: ctx.score_rows_pan([buf.data_ptr()] * 2, [8, 8], [0, 1], [0, 0], 16, buf.data_ptr() + 2050), "4-byte aligned"),
        ]:
            with pytest.raises(runtime.DuspHipError, match=needle) as e:
                call()
            assert e.value.status == -1
        assert not buf.cpu().numpy().any() and not out.any()  # (nothing ran)
        # and a mono piece with pans still renders on this context
        assert ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, pans=[-1, 1]).shape == (2, 128)
    finally:
        a.close()
        wide.close()
