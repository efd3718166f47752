"""Sub-sample onsets on the device (dusp_score_rows_frac_device, dusp_render_host_score_parts_frac): voices, each in a buffer of its own,
placed at onset + fraction samples through the reference Delay's two taps — bit for bit the numpy statement of the contract
(dusp_amd/mix.py score_chain_rows / score_chain_rows_panned with fracs), and, through render_piece(..., fracs=...), bit for bit the
oracle's render of the piece as ONE circuit whose Delay units take onset + fraction.  The kernel tests feed the planted rows of
tests/frac_cases.py, ONE ALLOCATION PER VOICE, and need no render.  Bit patterns everywhere (for NaN, the positions): no tolerances."""
import functools

import numpy as np
import pytest

import dusp_amd as d
import score_voices as sv
from conftest import knob_context
from dusp_amd import descriptor, render, runtime, wav
from dusp_amd.mix import score_chain_rows, score_chain_rows_panned
from frac_cases import as_one_frac_circuit, layout, pans_for, planted, planted_wide
from test_piece_host import NV_SAW, bits, interleaved_voice

pytestmark = pytest.mark.gpu

NT = 1301  # (five workgroups of 256 and 21 samples)
GUARD = 64  # floats in front of and behind the output
SENTINEL = np.float32(-12345.678)
COUNTS = [1, 8, 9, 37]  # a lone voice, one full batch of indices, one more, four batches and five
VARIANTS = ["plain", "gains", "init", "in_place"]
FORMS = {"block256": {}, "doubled_blocks": {"DUSP_SCORE_PLAN_KB": 1}}
KINDS = {"mono": (1, False), "wide": (2, False), "panned": (1, True)}  # channels of a row, panned


def frac_context(form):
    return knob_context(48000, **FORMS[form]) if FORMS[form] else render.context(48000)


def case(n, kind):
    return planted_wide(n, NT) if kind == "wide" else planted(n, NT)


@functools.lru_cache(maxsize=None)
def expected(n, kind, with_lengths, with_gains, with_init, raw, lo=0, hi=NT, with_fracs=True):
    """the contract over the window [lo, hi) of the timeline: the same chain with shifted onsets"""
    rows, onsets, lengths, gains, pans, init, fracs = case(n, kind)
    channels, panned = KINDS[kind]
    kw = dict(lengths=lengths if with_lengths else None, gains=gains if with_gains else None, raw=raw, fracs=fracs if with_fracs else None,
              init=np.ascontiguousarray(init[:2 if panned else channels, lo:hi]) if with_init else None)
    want = score_chain_rows_panned(rows, onsets - lo, pans, hi - lo, **kw) if panned else score_chain_rows(rows, onsets - lo, hi - lo, **kw)
    want.setflags(write=False)
    return want


def same(got, want, what):
    """bit patterns; for NaN, the positions"""
    nan = np.isnan(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), nan), what
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    assert np.array_equal(g, w), "%s: first differing sample %d of %d" % (what, int(np.argmax(g != w)), g.size)


@functools.lru_cache(maxsize=None)
def device_rows(n, kind):
    """every voice's row in an allocation of EXACTLY its floats behind 0, 1, 2 or 3 floats of offset; none at all for a row of no samples"""
    import torch
    rows = case(n, kind)[0]
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


def run_frac(ctx, n, kind, with_lengths=True, with_gains=False, init=None, raw=False, out_offset=0, lo=0, hi=NT, with_fracs=True):
    """init: None | "buffer" | "in_place".  out_offset: floats past a 16-byte boundary.  [lo, hi): the window of the timeline."""
    import torch
    rows, onsets, lengths, gains, pans, init_host, fracs = case(n, kind)
    channels, panned = KINDS[kind]
    out_ch = 2 if panned else channels
    nt = hi - lo
    row = out_ch * nt
    _, pointers = device_rows(n, kind)
    d_out = torch.full((GUARD + out_offset + row + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    at = GUARD + out_offset
    d_gains = torch.from_numpy(np.array(gains)).cuda() if with_gains else None
    d_init, p_init = None, None
    window = np.ascontiguousarray(init_host[:out_ch, lo:hi]).reshape(-1)
    if init == "in_place":
        d_out[at:at + row] = torch.from_numpy(window.copy()).cuda()
        p_init = d_out.data_ptr() + 4 * at
    elif init == "buffer":
        d_init = torch.from_numpy(window.copy()).cuda()
        p_init = d_init.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.score_rows_frac(pointers, [r.shape[1] for r in rows], channels, onsets - lo, fracs if with_fracs else None, nt, d_out.data_ptr() + 4 * at,
                        lengths if with_lengths else None, d_gains.data_ptr() if with_gains else None, p_init, raw, pans if panned else None, stream=stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    what = (n, kind, with_lengths, with_gains, init, raw, out_offset, lo, hi)
    assert np.array_equal(out[:at].view(np.uint32), np.full(at, SENTINEL).view(np.uint32)), "floats in front of the output were written: %r" % (what,)
    assert np.array_equal(out[at + row:].view(np.uint32), np.full(GUARD, SENTINEL).view(np.uint32)), "floats behind the output were written: %r" % (what,)
    got = out[at:at + row].reshape(out_ch, nt)
    same(got, expected(n, kind, with_lengths, with_gains, init is not None, bool(raw), lo, hi, with_fracs), what)
    return got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", COUNTS)
def test_score_rows_frac_equals_the_two_tap_chain(n, kind, variant, form):
    ctx = frac_context(form)
    for raw in (0, 1):
        if variant == "plain":
            run_frac(ctx, n, kind, raw=raw)
            run_frac(ctx, n, kind, with_lengths=False, raw=raw, out_offset=1)
        elif variant == "gains":
            run_frac(ctx, n, kind, with_gains=True, raw=raw, out_offset=2)
        elif variant == "init":
            run_frac(ctx, n, kind, with_gains=True, init="buffer", raw=raw)
            run_frac(ctx, n, kind, init="buffer", raw=raw)
        else:
            run_frac(ctx, n, kind, init="in_place", raw=raw)
            run_frac(ctx, n, kind, with_gains=True, init="in_place", raw=raw, out_offset=3)
    tensors, _ = device_rows(n, kind)
    for k, (t, r) in enumerate(zip(tensors, case(n, kind)[0])):
        assert t is None or np.array_equal(t[k % 4:].cpu().numpy().view(np.uint32), r.reshape(-1).view(np.uint32)), "a row was written to"


def test_the_planted_fractions_change_what_is_heard():
    """the expectations above are not the whole-sample chain's: the fractions matter, on every kind"""
    for kind in KINDS:
        a, b = expected(37, kind, True, True, False, True), expected(37, kind, True, True, False, True, with_fracs=False)
        assert (bits(a) != bits(b)).mean() > 0.3, kind


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_window_of_the_timeline_is_the_same_chain_with_shifted_onsets(kind, form):
    """window edges that are no multiples of 256: the pieces, raw and continued in place, are the whole timeline's bits"""
    ctx = frac_context(form)
    whole = expected(37, kind, True, True, True, True)
    pieces = [run_frac(ctx, 37, kind, with_gains=True, init="in_place", raw=True, out_offset=k % 4, lo=lo, hi=hi) for k, (lo, hi) in enumerate([(0, 300), (300, 1001), (1001, NT)])]
    same(np.concatenate(pieces, axis=1), whole, "windows")
    run_frac(ctx, 9, kind, init="buffer", lo=13, hi=899)


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_chain_cut_into_two_launches_and_continued_raw_is_the_whole(kind):
    """voices [0, 20) raw, then [20, 37) in place through init: what the tiles of a piece do"""
    import torch
    ctx = frac_context("block256")
    rows, onsets, lengths, gains, pans, _, fracs = case(37, kind)
    channels, panned = KINDS[kind]
    out_ch = 2 if panned else channels
    _, pointers = device_rows(37, kind)
    samples = [r.shape[1] for r in rows]
    d_out = torch.zeros(out_ch * NT, dtype=torch.float32, device="cuda")
    d_gains = torch.from_numpy(np.array(gains)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.score_rows_frac(pointers[:20], samples[:20], channels, onsets[:20], fracs[:20], NT, d_out.data_ptr(), lengths[:20], d_gains.data_ptr(), None, True,
                        pans[:20] if panned else None, stream=stream)
    ctx.score_rows_frac(pointers[20:], samples[20:], channels, onsets[20:], fracs[20:], NT, d_out.data_ptr(), lengths[20:], d_gains.data_ptr() + 4 * 20, d_out.data_ptr(), False,
                        pans[20:] if panned else None, stream=stream)
    torch.cuda.synchronize()
    kernel, plan, upload = ctx.score_last_ms()  # (dusp_score_last_ms reports the call)
    assert 0 < kernel < 1000 and 0 <= plan < 1000 and 0 < upload < 1000
    same(d_out.cpu().numpy().reshape(out_ch, NT), expected(37, kind, True, True, False, False), "two launches")


@pytest.mark.parametrize("kind", list(KINDS))
def test_all_fractions_zero_is_the_call_without_fractions_bit_for_bit(kind):
    """through the new entry point with zeros, and with no fractions at all: score_rows_device's / score_rows_pan's output"""
    import torch
    ctx = frac_context("block256")
    n = 37
    rows, onsets, lengths, gains, pans, init, _ = case(n, kind)
    channels, panned = KINDS[kind]
    out_ch = 2 if panned else channels
    _, pointers = device_rows(n, kind)
    samples = [r.shape[1] for r in rows]
    d_gains = torch.from_numpy(np.array(gains)).cuda()
    d_init = torch.from_numpy(np.ascontiguousarray(init[:out_ch]).reshape(-1).copy()).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for raw in (True, False):
        outs = []
        for fracs in ("old", np.zeros(n), None):
            d_out = torch.full((out_ch * NT,), float(SENTINEL), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            if isinstance(fracs, str) and panned:
                ctx.score_rows_pan(pointers, samples, onsets, pans, NT, d_out.data_ptr(), lengths, d_gains.data_ptr(), d_init.data_ptr(), raw, stream=stream)
            elif isinstance(fracs, str):
                ctx.score_rows_device(pointers, samples, channels, onsets, NT, d_out.data_ptr(), lengths, d_gains.data_ptr(), d_init.data_ptr(), raw, stream=stream)
            else:
                ctx.score_rows_frac(pointers, samples, channels, onsets, fracs, NT, d_out.data_ptr(), lengths, d_gains.data_ptr(), d_init.data_ptr(), raw,
                                    pans if panned else None, stream=stream)
            torch.cuda.synchronize()
            outs.append(d_out.cpu().numpy().reshape(out_ch, NT))
        same(outs[1], outs[0], "zeros")
        same(outs[2], outs[0], "None")
        same(outs[0], expected(n, kind, True, True, True, raw, with_fracs=False), "the chain without fractions")


def test_edge_voices_and_no_voices():
    """len = 1; onset = -1; onset = -len (the tail tap alone); onset + len = n_total (the tail tap clipped off); onset = n_total - 1; a
    first voice without a row; no voices at all — rows of exactly their size"""
    import torch
    ctx = render.context(48000)
    stream = torch.cuda.current_stream().cuda_stream
    row = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float32, device="cuda")
    host = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    d_out = torch.full((14,), 9.0, dtype=torch.float32, device="cuda")
    for onsets, lengths, fracs in (([2], [1], [0.25]), ([-1], [3], [0.25]), ([-3], [3], [0.75]), ([4], [3], [0.5]), ([6], [3], [0.5]), ([-4], [3], [0.5]), ([7], [3], [0.5])):
        ctx.score_rows_frac([row.data_ptr()], [3], 1, onsets, fracs, 7, d_out.data_ptr(), lengths, stream=stream)
        torch.cuda.synchronize()
        same(d_out.cpu().numpy()[:7].reshape(1, 7), score_chain_rows([host], onsets, 7, lengths, fracs=fracs), (onsets, lengths, fracs))
        ctx.score_rows_frac([row.data_ptr()], [3], 1, onsets, fracs, 7, d_out.data_ptr(), lengths, pans=[0.3], stream=stream)
        torch.cuda.synchronize()
        same(d_out.cpu().numpy().reshape(2, 7), score_chain_rows_panned([host], onsets, [0.3], 7, lengths, fracs=fracs), (onsets, lengths, fracs, "panned"))
    # voice 0 has no row at all (NULL, no samples) and a fraction, voice 1 three samples: the padded entries name voice 0
    ctx.score_rows_frac([None, row.data_ptr()], [0, 3], 1, [2, 3], [0.5, 0.5], 7, d_out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy()[:7].tolist() == [0, 0, 0, 0.5, 1.5, 2.5, 1.5]
    init = np.array([[1.0, -0.0, np.nan, 0.0, -2.5, np.inf, 1e-45], [-0.0, 3.0, 0.0, np.nan, -np.inf, 2.0, -1e-45]], dtype=np.float32)
    d_buf = torch.from_numpy(init.reshape(-1).copy()).cuda()
    ctx.score_rows_frac([], [], 1, [], [], 7, d_out.data_ptr(), d_init=d_buf.data_ptr(), raw=True, pans=[], stream=stream)
    torch.cuda.synchronize()
    same(d_out.cpu().numpy().reshape(2, 7), init, "raw: a copy of both channels")
    ctx.score_rows_frac([], [], 2, [], None, 7, d_out.data_ptr(), d_init=d_buf.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    same(d_out.cpu().numpy().reshape(2, 7), score_chain_rows([], [], 7, init=init), "`|| 0` of two channels")


# ---- dusp_render_host_score_parts_frac, render_piece(..., fracs=...) -----------------------------------------------------------------------

def voice_samples(n):
    return [sv.NV if k % 2 == 0 else NV_SAW for k in range(n)]


def piece_args(n, panned):
    rate = sv.SAMPLE_RATE
    onsets, fracs, gains = layout(n, panned)
    return onsets, fracs, gains, pans_for(n) if panned else None, [(s + 0.5) / rate for s in voice_samples(n)], (sv.NT + 0.5) / rate


@functools.lru_cache(maxsize=None)
def oracle_piece(n, panned, with_gains, oracle):
    """the oracle's render of the fractional piece as ONE circuit (tests/test_frac_host.py anchors the numpy contract to it)"""
    d.configure(sv.SAMPLE_RATE)
    onsets, fracs, gains, pans, _, _ = piece_args(n, panned)
    circuit = as_one_frac_circuit([interleaved_voice(k) for k in range(n)], onsets, fracs, gains if with_gains else None, pans)
    want = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("panned", [False, True], ids=["mono", "panned"])
@pytest.mark.parametrize("n", [2, 13, 37])
def test_render_piece_with_fracs_is_the_oracles_one_circuit(n, panned, with_gains, oracle):
    want = oracle_piece(n, panned, with_gains, oracle)
    assert want.shape == (2 if panned else 1, sv.NT)
    onsets, fracs, gains, pans, durations, dur = piece_args(n, panned)
    assert (fracs != 0).any()
    g = gains if with_gains else None
    d.configure(sv.SAMPLE_RATE)
    voices = lambda: [interleaved_voice(k) for k in range(n)]
    # tiles: the default (one), and 9000 bytes — two voices of 3092 and 4124 bytes a tile (two voices: a tile each)
    results = {}
    for tile_bytes in (0, 9000) if n > 2 else (0, 1):
        got = d.render_piece(voices(), onsets, durations, dur, None, g, tile_bytes=tile_bytes, pans=pans, fracs=fracs)
        assert got.sampleRate == sv.SAMPLE_RATE and len(got) == want.shape[0] and got[0].shape == (sv.NT,)
        results[tile_bytes] = np.stack(got)
    a, b = results.values()
    print("n %d panned %s gains %s: %d samples differ between the tilings, %d from the oracle" % (n, panned, with_gains, int((bits(a) != bits(b)).sum()), int((bits(a) != bits(want)).sum())))
    assert np.array_equal(bits(a), bits(b)), "the two tilings differ"
    for tile_bytes, got in results.items():
        assert np.array_equal(bits(got), bits(want)), (tile_bytes, "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0))))
    # and the piece with its onsets rounded is another piece: a voice with a fraction sounds for 700 samples, and nearly all of them differ
    rounded = np.stack(d.render_piece(voices(), onsets, durations, dur, None, g, pans=pans))
    assert (bits(rounded) != bits(want)).sum() >= 600


@pytest.mark.parametrize("panned", [False, True], ids=["mono", "panned"])
def test_render_score_with_fracs_is_render_piece_of_one_structure(panned, oracle):
    d.configure(sv.SAMPLE_RATE)
    n = 13
    _, lengths, _ = sv.layout(n)
    onsets, fracs, gains = layout(n, panned)
    pans = pans_for(n) if panned else None
    dur, voice_dur = (sv.NT + 0.5) / sv.SAMPLE_RATE, (sv.NV + 0.5) / sv.SAMPLE_RATE
    voices = lambda: [sv.voice(k) for k in range(n)]
    want = d.render_piece(voices(), onsets, voice_dur, dur, lengths, gains, pans=pans, fracs=fracs)
    got = d.render_score(voices(), onsets, voice_dur, dur, lengths, gains, pans=pans, fracs=fracs)
    assert got.sampleRate == want.sampleRate and len(got) == len(want) == (2 if panned else 1)
    assert np.array_equal(bits(np.stack(got)), bits(np.stack(want))) and np.abs(np.stack(got)).max() > 0
    # ... and, lengths only cutting off zeros, the oracle's one circuit of the score voices
    circuit = as_one_frac_circuit(voices(), onsets, fracs, gains, pans)
    ref = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
    assert np.array_equal(bits(np.stack(got)), bits(ref))
    assert len(d.render_score(voices(), onsets, voice_dur, 0, pans=pans, fracs=fracs)) == 0
    # all fractions zero: the score without fractions
    zeros = d.render_score(voices(), onsets, voice_dur, dur, lengths, gains, pans=pans, fracs=np.zeros(n))
    plain = d.render_score(voices(), onsets, voice_dur, dur, lengths, gains, pans=pans)
    assert np.array_equal(bits(np.stack(zeros)), bits(np.stack(plain)))
    # positions written as real numbers
    on2, fr2 = d.split_onsets(onsets + fracs)
    assert np.array_equal(on2, onsets) and np.array_equal(fr2, fracs)


def test_render_piece_pcm_and_wav_with_fracs():
    """s16 / s24 / f32 frames and the peak of the fractional panned piece: wav.encode_frames over the f32 result; the file."""
    n = 13
    rate = sv.SAMPLE_RATE
    d.configure(rate)
    onsets, fracs, gains, pans, durations, dur = piece_args(n, True)
    voices = lambda: [interleaved_voice(k) for k in range(n)]
    piece_f32 = np.stack(d.render_piece(voices(), onsets, durations, dur, None, gains, tile_bytes=20000, pans=pans, fracs=fracs))
    peak_want = np.float32(np.abs(piece_f32).max())
    assert piece_f32.shape == (2, sv.NT) and peak_want > 1.0  # (normalise = 1 has something to shrink)
    for depth, normalise in ((16, 0), (16, 1), (24, 2), (32, 0)):
        res = d.render_piece_pcm(voices(), onsets, durations, dur, depth, normalise, None, gains, tile_bytes=20000, pans=pans, fracs=fracs)
        want, want_peak = wav.encode_frames(piece_f32, depth, normalise)
        assert res.data.dtype == want.dtype and res.data.shape == want.shape and res.bitDepth == depth and res.numberOfChannels == 2
        assert np.array_equal(res.data.view(np.uint8), want.view(np.uint8)), (depth, normalise)
        assert np.float32(res.peak).view(np.uint32) == np.float32(want_peak).view(np.uint32) == peak_want.view(np.uint32)
    file = d.render_piece_wav(voices(), onsets, durations, dur, 16, 0, None, gains, pans=pans, fracs=fracs)
    assert file == wav.encode_wav([c for c in piece_f32], rate, 16) and file[:4] == b"RIFF"
    score_file = d.render_score_wav([sv.voice(k) for k in range(3)], [0, 10, 20], durations[0], dur, 16, 0, fracs=[0, 0.25, 0.5])
    score_f32 = np.stack(d.render_score([sv.voice(k) for k in range(3)], [0, 10, 20], durations[0], dur, fracs=[0, 0.25, 0.5]))
    assert score_f32.shape == (1, sv.NT) and score_file == wav.encode_wav([c for c in score_f32], rate, 16)


def test_refusals_on_a_live_context():
    import torch
    d.configure(sv.SAMPLE_RATE)
    ctx = knob_context(sv.SAMPLE_RATE, DUSP_WAVE_JIT=2)
    mono = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(2)])
    a = ctx.build(mono.words)
    try:
        for fracs, needle in (([0, float("nan")], "the fraction of voice 1 is not finite"), ([float("inf"), 0], "the fraction of voice 0 is not finite"),
                              ([0, 1.0], r"the fraction of voice 1 is outside \[0, 1\)"), ([-0.25, 0], r"the fraction of voice 0 is outside \[0, 1\)")):
            with pytest.raises(ValueError, match="dusp-hip: " + needle):
                ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, fracs=fracs)
        with pytest.raises(ValueError, match="fracs must have shape"):
            ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, fracs=[0])
        # the library's own checks, behind the binder's: bad fractions handed to the C calls
        buf = torch.zeros(1024, dtype=torch.float32, device="cuda")
        rows = np.array([buf.data_ptr(), buf.data_ptr()], dtype=np.uint64)
        samples, onsets = np.array([8, 8], dtype=np.uint32), np.array([0, 1], dtype=np.int64)
        pans = np.zeros(2, dtype=np.float32)
        table = (runtime.ScorePart * 1)(runtime.ScorePart(a._h, 2, 64, mono.params.ctypes.data if mono.params is not None else None))
        part_of, out = np.zeros(2, dtype=np.uint32), np.zeros((2, 128), dtype=np.float32)
        for bad, message in (([0.0, np.nan], b"the fraction of voice 1 is not finite"), ([-np.inf, 0.0], b"the fraction of voice 0 is not finite"),
                             ([0.5, 1.0], b"the fraction of voice 1 is outside [0, 1)"), ([-1e-300, 0.0], b"the fraction of voice 0 is outside [0, 1)")):
            bad = np.array(bad, dtype=np.float64)
            for p in (None, pans.ctypes.data):
                rc = ctx._L.dusp_score_rows_frac_device(ctx._h, rows.ctypes.data, samples.ctypes.data, 2, 1, onsets.ctypes.data, bad.ctypes.data, None, None, p, None, 16, None, 0,
                                                        buf.data_ptr() + 2048, None)
                assert rc == -1 and b"dusp_score_rows_frac_device: " + message in ctx._L.dusp_last_error(ctx._h)
                rc = ctx._L.dusp_render_host_score_parts_frac(table, 1, 2, part_of.ctypes.data, onsets.ctypes.data, bad.ctypes.data, None, None, p, None, 128, 0, 0, 0,
                                                              out.ctypes.data, None)
                assert rc == -1 and b"dusp_render_host_score_parts_frac: " + message in ctx._L.dusp_last_error(ctx._h)
        half = [0.5, 0.5]
        for call, needle in [
            (lambda: ctx.score_rows_frac([buf.data_ptr()] * 2, [8, 8], 2, [0, 1], half, 16, buf.data_ptr() + 2048, pans=[0, 0]), "a panned voice is mono: n_channels must be 1"),
            (lambda: ctx.score_rows_frac([buf.data_ptr()] * 2, [8, 8], 1, [0, 1], half, (1 << 30) + 1, buf.data_ptr() + 2048, pans=[0, 0]), "channels x timeline samples must not exceed 2\\^31"),
            (lambda: ctx.score_rows_frac([buf.data_ptr(), None], [8, 8], 1, [0, 1], half, 16, buf.data_ptr() + 2048), "dusp_score_rows_frac_device: the row of voice 1 is NULL"),
            (lambda: ctx.score_rows_frac([buf.data_ptr()] * 2, [8, 4], 1, [0, 1], half, 16, buf.data_ptr() + 2048, lengths=[8, 5]), "length of voice 1 is 5"),
            (lambda: ctx.score_rows_frac([buf.data_ptr()] * 2, [8, 8], 1, [0, 1], half, 16, buf.data_ptr() + 2050), "4-byte aligned"),
            (lambda: ctx.score_rows_frac([buf.data_ptr()] * 2, [8, 8], 1, [0, 1], half, 16, buf.data_ptr() + 2048, pans=[0, float("nan")]), None),
        ]:
            with pytest.raises((runtime.DuspHipError, ValueError), match=needle) as e:
                call()
            assert needle is None or e.value.status == -1
        with pytest.raises(ValueError, match="onsets are in samples, whole numbers"):
            ctx.score_rows_frac([buf.data_ptr()] * 2, [8, 8], 1, [0, 0.5], half, 16, buf.data_ptr() + 2048)
        assert not buf.cpu().numpy().any() and not out.any()  # (nothing ran)
        # and a piece with fractions still renders on this context, with and without pans
        assert ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, fracs=[0.5, 0.25]).shape == (1, 128)
        assert ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, pans=[-1, 1], fracs=[0.5, 0.25]).shape == (2, 128)
    finally:
        a.close()
