"""Space placement on the device (dusp_score_rows_space_device, dusp_render_host_score_parts_space): mono voices, each in a buffer of its
own, heard by every speaker through a gain and a delay of their own — bit for bit the numpy statement of the contract (dusp_amd/mix.py
score_chain_rows_placed), and, through render_piece(..., places=...), bit for bit the oracle's render of the anchor circuit channel by
channel (tests/space_cases.py).  The kernel tests feed the planted rows of tests/space_cases.py, ONE ALLOCATION PER VOICE, and need no
render.  Bit patterns everywhere (for NaN, the positions): no tolerances."""
import functools

import numpy as np
import pytest

import dusp_amd as d
import score_voices as sv
from conftest import knob_context
from dusp_amd import descriptor, render, runtime, wav
from dusp_amd.mix import score_chain_rows, score_chain_rows_placed
from space_cases import EDGE_DELAYS, SDPM, SPEAKERS, anchor_circuit, decibels, layout, planted
from test_piece_host import NV_SAW, bits, interleaved_voice

pytestmark = pytest.mark.gpu

NT = 1301  # (five workgroups of 256 and 21 samples)
GUARD = 64  # floats in front of and behind the output
SENTINEL = np.float32(-12345.678)
COUNTS = [1, 8, 9, 37]  # a lone voice, one full batch of indices, one more, four batches and five
SPEAKER_COUNTS = [1, 2, 3, 6]
VARIANTS = ["plain", "gains", "init", "in_place"]
FORMS = {"block256": {}, "doubled_blocks": {"DUSP_SCORE_PLAN_KB": 1}}


def space_context(form):
    return knob_context(48000, **FORMS[form]) if FORMS[form] else render.context(48000)


@functools.lru_cache(maxsize=None)
def expected(n, n_speakers, with_lengths, with_gains, with_init, raw, lo=0, hi=NT):
    """the contract over the window [lo, hi) of the timeline: the same chain with shifted onsets"""
    rows, onsets, lengths, gains, delays, tap_gains, init = planted(n, n_speakers, NT)
    want = score_chain_rows_placed(rows, onsets - lo, delays, tap_gains, hi - lo, lengths=lengths if with_lengths else None, gains=gains if with_gains else None, raw=raw,
                                   init=np.ascontiguousarray(init[:, lo:hi]) if with_init else None)
    want.setflags(write=False)
    return want


def same(got, want, what):
    """bit patterns; for NaN, the positions"""
    nan = np.isnan(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), nan), what
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    assert np.array_equal(g, w), "%s: first differing sample %d of %d" % (what, int(np.argmax(g != w)), g.size)


@functools.lru_cache(maxsize=None)
def device_rows(n):
    """every voice's row in an allocation of EXACTLY its floats behind 0, 1, 2 or 3 floats of offset; none at all for a row of no samples
    (the rows do not depend on the speakers)"""
    import torch
    rows = planted(n, 1, NT)[0]
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


def run_space(ctx, n, n_speakers, with_lengths=True, with_gains=False, init=None, raw=False, out_offset=0, lo=0, hi=NT):
    """init: None | "buffer" | "in_place".  out_offset: floats past a 16-byte boundary.  [lo, hi): the window of the timeline."""
    import torch
    rows, onsets, lengths, gains, delays, tap_gains, init_host = planted(n, n_speakers, NT)
    nt = hi - lo
    row = n_speakers * nt
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
    ctx.score_rows_space(pointers, [r.shape[1] for r in rows], onsets - lo, delays, tap_gains, nt, d_out.data_ptr() + 4 * at, lengths if with_lengths else None,
                         d_gains.data_ptr() if with_gains else None, p_init, raw, stream=stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    what = (n, n_speakers, with_lengths, with_gains, init, raw, out_offset, lo, hi)
    assert np.array_equal(out[:at].view(np.uint32), np.full(at, SENTINEL).view(np.uint32)), "floats in front of the output were written: %r" % (what,)
    assert np.array_equal(out[at + row:].view(np.uint32), np.full(GUARD, SENTINEL).view(np.uint32)), "floats behind the output were written: %r" % (what,)
    got = out[at:at + row].reshape(n_speakers, nt)
    same(got, expected(n, n_speakers, with_lengths, with_gains, init is not None, bool(raw), lo, hi), what)
    return got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n_speakers", SPEAKER_COUNTS)
@pytest.mark.parametrize("n", COUNTS)
def test_score_rows_space_equals_the_placed_chain(n, n_speakers, variant, form):
    ctx = space_context(form)
    for raw in (0, 1):
        if variant == "plain":
            run_space(ctx, n, n_speakers, raw=raw)
            run_space(ctx, n, n_speakers, with_lengths=False, raw=raw, out_offset=1)
        elif variant == "gains":
            run_space(ctx, n, n_speakers, with_gains=True, raw=raw, out_offset=2)
        elif variant == "init":
            run_space(ctx, n, n_speakers, with_gains=True, init="buffer", raw=raw)
        else:
            run_space(ctx, n, n_speakers, with_gains=True, init="in_place", raw=raw, out_offset=3)
    tensors, _ = device_rows(n)
    for k, (t, r) in enumerate(zip(tensors, planted(n, 1, NT)[0])):
        assert t is None or np.array_equal(t[k % 4:].cpu().numpy().view(np.uint32), r.reshape(-1).view(np.uint32)), "a row was written to"


def test_the_planted_taps_hold_what_they_are_built_to_hold():
    """every edge delay is among the taps; one channel's span lies wholly outside the window while the voice's others are inside; the
    fractions are heard"""
    rows, onsets, lengths, gains, delays, tap_gains, _ = planted(37, 3, NT)
    assert set(EDGE_DELAYS) <= set(delays.ravel().tolist()) and {0.0, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -53, 255.0, 256.25, 1300.5} == set(EDGE_DELAYS)
    k = 2
    assert lengths[k] > 0 and onsets[k] + delays[k, 1] >= NT and -lengths[k] < onsets[k] + delays[k, 0] < NT
    a = expected(37, 3, True, True, False, True)
    b = score_chain_rows_placed(rows, onsets, np.floor(delays), tap_gains, NT, lengths=lengths, gains=gains, raw=True)
    assert (bits(a) != bits(b)).mean() > 0.2


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n_speakers", [2, 3])
def test_a_window_of_the_timeline_is_the_same_chain_with_shifted_onsets(n_speakers, form):
    """window edges that are no multiples of 256: the pieces, raw and continued in place, are the whole timeline's bits"""
    ctx = space_context(form)
    whole = expected(37, n_speakers, True, True, True, True)
    pieces = [run_space(ctx, 37, n_speakers, with_gains=True, init="in_place", raw=True, out_offset=k % 4, lo=lo, hi=hi) for k, (lo, hi) in enumerate([(0, 300), (300, 1001), (1001, NT)])]
    same(np.concatenate(pieces, axis=1), whole, "windows")
    run_space(ctx, 9, n_speakers, init="buffer", lo=13, hi=899)


@pytest.mark.parametrize("n_speakers", [2, 6])
def test_the_chain_cut_into_two_launches_and_continued_raw_is_the_whole(n_speakers):
    """voices [0, 20) raw, then [20, 37) in place through init: what the tiles of a piece do"""
    import torch
    ctx = space_context("block256")
    rows, onsets, lengths, gains, delays, tap_gains, _ = planted(37, n_speakers, NT)
    _, pointers = device_rows(37)
    samples = [r.shape[1] for r in rows]
    d_out = torch.zeros(n_speakers * NT, dtype=torch.float32, device="cuda")
    d_gains = torch.from_numpy(np.array(gains)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.score_rows_space(pointers[:20], samples[:20], onsets[:20], delays[:20], tap_gains[:20], NT, d_out.data_ptr(), lengths[:20], d_gains.data_ptr(), None, True, stream=stream)
    ctx.score_rows_space(pointers[20:], samples[20:], onsets[20:], delays[20:], tap_gains[20:], NT, d_out.data_ptr(), lengths[20:], d_gains.data_ptr() + 4 * 20, d_out.data_ptr(), False,
                         stream=stream)
    torch.cuda.synchronize()
    kernel, plan, upload = ctx.score_last_ms()  # (dusp_score_last_ms reports the call)
    assert 0 < kernel < 1000 and 0 <= plan < 1000 and 0 < upload < 1000
    same(d_out.cpu().numpy().reshape(n_speakers, NT), expected(37, n_speakers, True, True, False, False), "two launches")


@pytest.mark.parametrize("n_speakers", [1, 3])
def test_every_delay_zero_and_every_gain_one_is_the_rows_call_on_each_channel(n_speakers):
    """through the new entry point: score_rows_device's output, channel by channel"""
    import torch
    ctx = space_context("block256")
    n = 37
    rows, onsets, lengths, gains, _, _, init = planted(n, n_speakers, NT)
    _, pointers = device_rows(n)
    samples = [r.shape[1] for r in rows]
    d_gains = torch.from_numpy(np.array(gains)).cuda()
    d_init = torch.from_numpy(np.ascontiguousarray(init).reshape(-1).copy()).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    zeros, ones = np.zeros((n, n_speakers)), np.ones((n, n_speakers))
    for raw in (True, False):
        d_out = torch.full((n_speakers * NT,), float(SENTINEL), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.score_rows_space(pointers, samples, onsets, zeros, ones, NT, d_out.data_ptr(), lengths, d_gains.data_ptr(), d_init.data_ptr(), raw, stream=stream)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().reshape(n_speakers, NT)
        for c in range(n_speakers):
            d_one = torch.full((NT,), float(SENTINEL), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ctx.score_rows_device(pointers, samples, 1, onsets, NT, d_one.data_ptr(), lengths, d_gains.data_ptr(), d_init.data_ptr() + 4 * c * NT, raw, stream=stream)
            torch.cuda.synchronize()
            same(got[c:c + 1], d_one.cpu().numpy().reshape(1, NT), ("rows call", raw, c))
            same(got[c:c + 1], score_chain_rows(rows, onsets, NT, lengths, gains, init=init[c:c + 1], raw=raw), ("mono chain", raw, c))


def test_edge_voices_and_no_voices():
    """len = 1; a tail tap alone on sample 0; a tail tap clipped off; a delay past the timeline; a first voice without a row; no voices
    at all — rows of exactly their size"""
    import torch
    ctx = render.context(48000)
    stream = torch.cuda.current_stream().cuda_stream
    row = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float32, device="cuda")
    host = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    d_out = torch.full((14,), 9.0, dtype=torch.float32, device="cuda")
    for onsets, lengths, delays in (([2], [1], [[0.25, 0.0]]), ([-1], [3], [[0.25, 1.0]]), ([-3], [3], [[0.75, 0.0]]), ([-4], [3], [[1.5, 0.5]]), ([4], [3], [[0.5, 3.0]]), ([0], [3], [[6.5, 7.0]]),
                                    ([-4], [3], [[0.5, 2.0 ** 24]]), ([7], [3], [[0.5, 0.0]])):
        tap_gains = [[1.0, -0.5]]
        ctx.score_rows_space([row.data_ptr()], [3], onsets, delays, tap_gains, 7, d_out.data_ptr(), lengths, stream=stream)
        torch.cuda.synchronize()
        same(d_out.cpu().numpy().reshape(2, 7), score_chain_rows_placed([host], onsets, delays, tap_gains, 7, lengths), (onsets, lengths, delays))
    # voice 0 has no row at all (NULL, no samples), voice 1 three samples: the padded entries name voice 0
    ctx.score_rows_space([None, row.data_ptr()], [0, 3], [2, 3], [[0.5], [0.5]], [[1.0], [1.0]], 7, d_out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy()[:7].tolist() == [0, 0, 0, 0.5, 1.5, 2.5, 1.5]
    init = np.array([[1.0, -0.0, np.nan, 0.0, -2.5, np.inf, 1e-45], [-0.0, 3.0, 0.0, np.nan, -np.inf, 2.0, -1e-45]], dtype=np.float32)
    d_buf = torch.from_numpy(init.reshape(-1).copy()).cuda()
    ctx.score_rows_space([], [], [], np.zeros((0, 2)), np.zeros((0, 2)), 7, d_out.data_ptr(), d_init=d_buf.data_ptr(), raw=True, stream=stream)
    torch.cuda.synchronize()
    same(d_out.cpu().numpy().reshape(2, 7), init, "raw: a copy of both channels")
    ctx.score_rows_space([], [], [], np.zeros((0, 2)), np.zeros((0, 2)), 7, d_out.data_ptr(), d_init=d_buf.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    same(d_out.cpu().numpy().reshape(2, 7), score_chain_rows([], [], 7, init=init), "`|| 0` of two channels")


# ---- dusp_render_host_score_parts_space, render_piece(..., places=...) ---------------------------------------------------------------------

def voice_samples(n):
    return [sv.NV if k % 2 == 0 else NV_SAW for k in range(n)]


def piece_args(n, n_speakers):
    rate = sv.SAMPLE_RATE
    onsets, gains, places, speakers, delays, tap_gains = layout(n, n_speakers)
    return onsets, gains, places, speakers, delays, [(s + 0.5) / rate for s in voice_samples(n)], (sv.NT + 0.5) / rate


@functools.lru_cache(maxsize=None)
def oracle_piece(n, n_speakers, with_gains, interleave, oracle):
    """the oracle's render of the anchor circuit, channel by channel (tests/test_space_host.py anchors the numpy contract to it)"""
    d.configure(sv.SAMPLE_RATE)
    onsets, gains, places, speakers, delays, _, _ = piece_args(n, n_speakers)
    db = decibels(places, speakers)
    voice = interleaved_voice if interleave else sv.voice
    want = np.concatenate([np.asarray(oracle.render(descriptor.extract(anchor_circuit([voice(k) for k in range(n)], onsets, db, delays, c, gains if with_gains else None)).words, sv.NT),
                                      dtype=np.float32) for c in range(n_speakers)])
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("n,n_speakers", [(2, 2), (13, 2), (13, 3)])
def test_render_piece_with_places_is_the_oracles_anchor_channel_by_channel(n, n_speakers, with_gains, oracle):
    want = oracle_piece(n, n_speakers, with_gains, True, oracle)
    assert want.shape == (n_speakers, sv.NT)
    onsets, gains, places, speakers, delays, durations, dur = piece_args(n, n_speakers)
    assert (delays != np.floor(delays)).any() and delays[0, 0] == 0 and delays[1, 1] == 256
    g = gains if with_gains else None
    d.configure(sv.SAMPLE_RATE)
    voices = lambda: [interleaved_voice(k) for k in range(n)]
    # tiles: the default (one), and 9000 bytes — two voices of 3092 and 4124 bytes a tile (two voices: a tile each)
    results = {}
    for tile_bytes in (0, 9000) if n > 2 else (0, 1):
        got = d.render_piece(voices(), onsets, durations, dur, None, g, tile_bytes=tile_bytes, places=places, speakers=speakers, sample_delay_per_metre=SDPM)
        assert got.sampleRate == sv.SAMPLE_RATE and len(got) == n_speakers and got[0].shape == (sv.NT,)
        results[tile_bytes] = np.stack(got)
    a, b = results.values()
    print("n %d speakers %d gains %s: %d samples differ between the tilings, %d from the oracle" % (n, n_speakers, with_gains, int((bits(a) != bits(b)).sum()), int((bits(a) != bits(want)).sum())))
    assert np.array_equal(bits(a), bits(b)), "the two tilings differ"
    for tile_bytes, got in results.items():
        assert np.array_equal(bits(got), bits(want)), (tile_bytes, "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0))))
    # other places are another piece
    moved = np.array(places) + np.float32(0.01)
    assert (bits(np.stack(d.render_piece(voices(), onsets, durations, dur, None, g, places=moved, speakers=speakers, sample_delay_per_metre=SDPM))) != bits(want)).sum() >= 600


def test_render_score_with_places_is_render_piece_of_one_structure(oracle):
    d.configure(sv.SAMPLE_RATE)
    n = 13
    _, lengths, _ = sv.layout(n)
    onsets, gains, places, speakers, delays, _, dur = piece_args(n, 2)
    voice_dur = (sv.NV + 0.5) / sv.SAMPLE_RATE
    voices = lambda: [sv.voice(k) for k in range(n)]
    kw = dict(places=places, speakers=speakers, sample_delay_per_metre=SDPM)
    want = d.render_piece(voices(), onsets, voice_dur, dur, lengths, gains, **kw)
    got = d.render_score(voices(), onsets, voice_dur, dur, lengths, gains, **kw)
    assert got.sampleRate == want.sampleRate and len(got) == len(want) == 2
    assert np.array_equal(bits(np.stack(got)), bits(np.stack(want))) and np.abs(np.stack(got)).max() > 0
    # ... and, lengths only cutting off zeros, the oracle's anchor circuits of the score voices
    assert np.array_equal(bits(np.stack(got)), bits(oracle_piece(n, 2, True, False, oracle)))
    assert len(d.render_score(voices(), onsets, voice_dur, 0, **kw)) == 0
    # every note on the one speaker at the origin, no attenuation: the mono score
    here = d.render_score(voices(), onsets, voice_dur, dur, lengths, gains, places=[[0, 0]] * n, speakers=[[0, 0]])
    plain = d.render_score(voices(), onsets, voice_dur, dur, lengths, gains)
    assert len(here) == 1 and np.array_equal(bits(np.stack(here)), bits(np.stack(plain)))
    # the default speakers and factors: the reference's stereo pair, -3 dB and sample rate / 343 samples a metre
    default = np.stack(d.render_score(voices(), onsets, voice_dur, dur, lengths, gains, places=places))
    spelt = np.stack(d.render_score(voices(), onsets, voice_dur, dur, lengths, gains, places=places, speakers=[[-1, 0], [1, 0]], decibels_per_metre=-3,
                                    sample_delay_per_metre=sv.SAMPLE_RATE / 343))
    assert default.shape == (2, sv.NT) and np.array_equal(bits(default), bits(spelt)) and not np.array_equal(bits(default), bits(np.stack(got)))


def test_render_piece_pcm_and_wav_with_places():
    """s16 / s24 / f32 frames and the peak of the placed piece on three speakers: wav.encode_frames over the f32 result; the file."""
    n = 13
    rate = sv.SAMPLE_RATE
    d.configure(rate)
    onsets, gains, places, speakers, _, durations, dur = piece_args(n, 3)
    kw = dict(places=places, speakers=speakers, sample_delay_per_metre=SDPM)
    voices = lambda: [interleaved_voice(k) for k in range(n)]
    piece_f32 = np.stack(d.render_piece(voices(), onsets, durations, dur, None, gains, tile_bytes=20000, **kw))
    peak_want = np.float32(np.abs(piece_f32).max())
    assert piece_f32.shape == (3, sv.NT) and peak_want > 1.0  # (normalise = 1 has something to shrink)
    for depth, normalise in ((16, 0), (16, 1), (24, 2), (32, 0)):
        res = d.render_piece_pcm(voices(), onsets, durations, dur, depth, normalise, None, gains, tile_bytes=20000, **kw)
        want, want_peak = wav.encode_frames(piece_f32, depth, normalise)
        assert res.data.dtype == want.dtype and res.data.shape == want.shape and res.bitDepth == depth and res.numberOfChannels == 3
        assert np.array_equal(res.data.view(np.uint8), want.view(np.uint8)), (depth, normalise)
        assert np.float32(res.peak).view(np.uint32) == np.float32(want_peak).view(np.uint32) == peak_want.view(np.uint32)
    file = d.render_piece_wav(voices(), onsets, durations, dur, 16, 0, None, gains, **kw)
    assert file == wav.encode_wav([c for c in piece_f32], rate, 16) and file[:4] == b"RIFF"
    few = dict(places=[[0, 0], [1, 1], [-2, 0.5]])
    score_file = d.render_score_wav([sv.voice(k) for k in range(3)], [0, 10, 20], durations[0], dur, 16, 0, **few)
    score_f32 = np.stack(d.render_score([sv.voice(k) for k in range(3)], [0, 10, 20], durations[0], dur, **few))
    assert score_f32.shape == (2, sv.NT) and score_file == wav.encode_wav([c for c in score_f32], rate, 16)


def test_refusals_on_a_live_context():
    import torch
    d.configure(sv.SAMPLE_RATE)
    ctx = knob_context(sv.SAMPLE_RATE, DUSP_WAVE_JIT=2)
    mono = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(2)])
    a = ctx.build(mono.words)
    try:
        ok = [[0.0, 1.5], [2.0, 0.0]]
        for taps, needle in (((ok, [[1.0, 1.0], [1.0, float("nan")]]), "the gain of voice 1 at speaker 1 is not finite"), (([[0.0, -1.0], [0.0, 0.0]], ok), r"the delay of voice 0 at speaker 1 is outside \[0, 2\^24\] samples"),
                             (([[0.0, 0.0], [float("inf"), 0.0]], ok), "the delay of voice 1 at speaker 0 is not finite")):
            with pytest.raises(ValueError, match="dusp-hip: " + needle):
                ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, taps=taps)
        with pytest.raises(ValueError, match="places stand alone"):
            ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, taps=(ok, ok), fracs=[0, 0])
        # the library's own checks, behind the binder's: bad taps handed to the C calls
        buf = torch.zeros(1024, dtype=torch.float32, device="cuda")
        rows = np.array([buf.data_ptr(), buf.data_ptr()], dtype=np.uint64)
        samples, onsets = np.array([8, 8], dtype=np.uint32), np.array([0, 1], dtype=np.int64)
        table = (runtime.ScorePart * 1)(runtime.ScorePart(a._h, 2, 64, mono.params.ctypes.data if mono.params is not None else None))
        part_of, out = np.zeros(2, dtype=np.uint32), np.zeros((2, 128), dtype=np.float32)
        good = np.array(ok, dtype=np.float64)
        for delays, gains, speakers, message in (([[0.0, np.nan], [0, 0]], ok, 2, b"the delay of voice 0 at speaker 1 is not finite"),
                                                 ([[0.0, 0.0], [2.0 ** 24 + 2, 0]], ok, 2, b"the delay of voice 1 at speaker 0 is outside [0, 2^24] samples"),
                                                 ([[0.0, 0.0], [0, -1e-300]], ok, 2, b"the delay of voice 1 at speaker 1 is outside [0, 2^24] samples"),
                                                 (ok, [[1.0, -np.inf], [1, 1]], 2, b"the gain of voice 0 at speaker 1 is not finite"),
                                                 (ok, ok, 0, b"a Space has 1 .. 8 speakers, not 0"), (ok, ok, 9, b"a Space has 1 .. 8 speakers, not 9"),
                                                 (None, ok, 2, b"the taps' delays or gains are NULL"), (ok, None, 2, b"the taps' delays or gains are NULL")):
            dl = None if delays is None else np.array(delays, dtype=np.float64)
            tg = None if gains is None else np.array(gains, dtype=np.float64)
            p_dl, p_tg = (None if dl is None else dl.ctypes.data), (None if tg is None else tg.ctypes.data)
            rc = ctx._L.dusp_score_rows_space_device(ctx._h, rows.ctypes.data, samples.ctypes.data, 2, speakers, onsets.ctypes.data, None, None, p_dl, p_tg, 16, None, 0,
                                                     buf.data_ptr() + 2048, None)
            assert rc == -1 and b"dusp_score_rows_space_device: " + message in ctx._L.dusp_last_error(ctx._h)
            rc = ctx._L.dusp_render_host_score_parts_space(table, 1, 2, part_of.ctypes.data, onsets.ctypes.data, None, None, speakers, p_dl, p_tg, 128, 0, 0, 0, out.ctypes.data, None)
            assert rc == -1 and b"dusp_render_host_score_parts_space: " + message in ctx._L.dusp_last_error(ctx._h)
        rc = ctx._L.dusp_score_rows_space_device(ctx._h, rows.ctypes.data, samples.ctypes.data, 2, 2, onsets.ctypes.data, None, None, good.ctypes.data, good.ctypes.data, (1 << 30) + 1, None, 0,
                                                 buf.data_ptr() + 2048, None)
        assert rc == -1 and b"speakers x timeline samples must not exceed 2^31" in ctx._L.dusp_last_error(ctx._h)
        for call, needle in [
            (lambda: ctx.score_rows_space([buf.data_ptr(), None], [8, 8], [0, 1], ok, ok, 16, buf.data_ptr() + 2048), "dusp_score_rows_space_device: the row of voice 1 is NULL"),
            (lambda: ctx.score_rows_space([buf.data_ptr()] * 2, [8, 4], [0, 1], ok, ok, 16, buf.data_ptr() + 2048, lengths=[8, 5]), "length of voice 1 is 5"),
            (lambda: ctx.score_rows_space([buf.data_ptr()] * 2, [8, 8], [0, 1], ok, ok, 16, buf.data_ptr() + 2050), "4-byte aligned"),
        ]:
            with pytest.raises(runtime.DuspHipError, match=needle) as e:
                call()
            assert e.value.status == -1
        stereo = descriptor.unify([descriptor.extract(d.Pan(sv.voice(k), 0.25)) for k in range(2)])
        b = ctx.build(stereo.words)
        try:
            with pytest.raises(runtime.DuspHipError, match="a placed voice is mono"):
                ctx.render_score_parts([(b, 64, 2, stereo.params)], [0, 0], [0, 1], 128, taps=(ok, ok))
        finally:
            b.close()
        with pytest.raises(ValueError, match="onsets are in samples, whole numbers"):
            ctx.score_rows_space([buf.data_ptr()] * 2, [8, 8], [0, 0.5], ok, ok, 16, buf.data_ptr() + 2048)
        assert not buf.cpu().numpy().any() and not out.any()  # (nothing ran)
        # and a placed piece still renders on this context
        assert ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, taps=(ok, ok)).shape == (2, 128)
        assert ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, taps=([[0.5] * 6] * 2, [[1.0] * 6] * 2)).shape == (6, 128)
    finally:
        a.close()
