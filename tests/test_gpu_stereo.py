"""Stereo pieces on the device (dusp_score_rows_stereo_device, dusp_render_host_score_parts_stereo): panned mono voices, plain mono voices
and voices of two channels side by side, each in a buffer of its own, added to a two-channel timeline — bit for bit the numpy statement
of the contract (dusp_amd/mix.py score_chain_rows_stereo), bit for bit the existing pan and rows calls where every voice is of their
kind, and, through render_piece(..., stereo=True), bit for bit the oracle's render of the piece as ONE circuit.  The kernel tests feed
the planted rows of tests/stereo_cases.py, ONE ALLOCATION PER VOICE of exactly channels x samples floats, and need no render."""
import functools

import numpy as np
import pytest

import dusp_amd as d
import score_voices as sv
import stereo_cases as sc
from conftest import knob_context
from dusp_amd import descriptor, render, runtime, wav
from dusp_amd.mix import score_chain_rows_stereo
from test_piece_host import bits

pytestmark = pytest.mark.gpu

NT = 1301  # (five workgroups of 256 and 21 samples)
GUARD = 64  # floats in front of and behind the output
SENTINEL = np.float32(-12345.678)
COUNTS = [1, 8, 9, 37]  # a lone voice, one full batch of the kernel's depth, one more, four batches and five
VARIANTS = ["plain", "gains", "init", "in_place"]
FORMS = {"union_window": {}, "doubled_blocks": {"DUSP_SCORE_PLAN_KB": 1}}


def stereo_context(form):
    return knob_context(48000, **FORMS[form]) if FORMS[form] else render.context(48000)


@functools.lru_cache(maxsize=None)
def expected(n, kinds, with_lengths, with_gains, with_init, raw, with_fracs, lo=0, hi=NT):
    """the contract over the window [lo, hi) of the timeline: the same chain with shifted onsets"""
    rows, onsets, lengths, gains, pans, init, fracs = sc.planted(n, NT, kinds)
    want = score_chain_rows_stereo(rows, onsets - lo, pans, hi - lo, lengths if with_lengths else None, gains if with_gains else None,
                                   np.ascontiguousarray(init[:, lo:hi]) if with_init else None, raw, fracs=fracs if with_fracs else None)
    want.setflags(write=False)
    return want


def same(got, want, what):
    """bit patterns; for NaN, the positions"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    assert np.array_equal(g, w), "%s: first differing sample %d of %d" % (what, int(np.argmax(g != w)), g.size)


@functools.lru_cache(maxsize=None)
def device_rows(n, kinds="in_turn"):
    """every voice's row in an allocation of its own, 0, 4, 8 or 12 bytes past a 16-byte boundary; none at all for a row of no samples"""
    import torch
    rows = sc.planted(n, NT, kinds)[0]
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


def run_stereo(ctx, n, kinds="in_turn", with_lengths=True, with_gains=False, init=None, raw=False, with_fracs=False, out_offset=0, lo=0, hi=NT):
    """init: None | "buffer" | "in_place".  out_offset: floats past a 16-byte boundary.  [lo, hi): the window of the timeline."""
    import torch
    rows, onsets, lengths, gains, pans, init_host, fracs = sc.planted(n, NT, kinds)
    nt = hi - lo
    row = 2 * nt
    _, pointers = device_rows(n, kinds)
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
    ctx.score_rows_stereo(pointers, [r.shape[1] for r in rows], [r.shape[0] for r in rows], onsets - lo, pans, nt, d_out.data_ptr() + 4 * at, lengths if with_lengths else None,
                          d_gains.data_ptr() if with_gains else None, p_init, raw, fracs=fracs if with_fracs else None, stream=stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    what = (n, kinds, with_lengths, with_gains, init, raw, with_fracs, out_offset, lo, hi)
    assert np.array_equal(out[:at].view(np.uint32), np.full(at, SENTINEL).view(np.uint32)), "floats in front of the output were written: %r" % (what,)
    assert np.array_equal(out[at + row:].view(np.uint32), np.full(GUARD, SENTINEL).view(np.uint32)), "floats behind the output were written: %r" % (what,)
    got = out[at:at + row].reshape(2, nt)
    same(got, expected(n, kinds, with_lengths, with_gains, init is not None, bool(raw), with_fracs, lo, hi), what)
    return got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", COUNTS)
def test_score_rows_stereo_equals_the_stereo_chain(n, variant, form):
    """the planted rows, kinds in turn; fractions 0, 0.5, 2^-24 and 1 - 2^-53 (and others) mixed in one list; init with -0, inf and NaN"""
    ctx = stereo_context(form)
    for with_fracs in (False, True):
        for raw in (0, 1):
            if variant == "plain":
                run_stereo(ctx, n, raw=raw, with_fracs=with_fracs)
                run_stereo(ctx, n, with_lengths=False, raw=raw, with_fracs=with_fracs, out_offset=1)
            elif variant == "gains":
                run_stereo(ctx, n, with_gains=True, raw=raw, with_fracs=with_fracs, out_offset=2)
            elif variant == "init":
                run_stereo(ctx, n, with_gains=True, init="buffer", raw=raw, with_fracs=with_fracs)
                run_stereo(ctx, n, init="buffer", raw=raw, with_fracs=with_fracs)
            else:
                run_stereo(ctx, n, init="in_place", raw=raw, with_fracs=with_fracs)
                run_stereo(ctx, n, with_gains=True, init="in_place", raw=raw, with_fracs=with_fracs, out_offset=3)
    tensors, _ = device_rows(n)
    for k, (t, r) in enumerate(zip(tensors, sc.planted(n, NT)[0])):
        assert t is None or np.array_equal(t[k % 4:].cpu().numpy().view(np.uint32), r.reshape(-1).view(np.uint32)), "a row was written to"


@pytest.mark.parametrize("with_fracs", [False, True], ids=["whole", "fracs"])
@pytest.mark.parametrize("form", list(FORMS))
def test_a_window_of_the_timeline_is_the_same_chain_with_shifted_onsets(form, with_fracs):
    """window edges that are no multiples of 256: the pieces, raw and continued in place, are the whole timeline's bits"""
    ctx = stereo_context(form)
    whole = expected(37, "in_turn", True, True, True, True, with_fracs)
    pieces = [run_stereo(ctx, 37, with_gains=True, init="in_place", raw=True, with_fracs=with_fracs, out_offset=k % 4, lo=lo, hi=hi)
              for k, (lo, hi) in enumerate([(0, 300), (300, 1001), (1001, NT)])]
    same(np.concatenate(pieces, axis=1), whole, "windows")
    run_stereo(ctx, 9, init="buffer", with_fracs=with_fracs, lo=13, hi=899)


@pytest.mark.parametrize("with_fracs", [False, True], ids=["whole", "fracs"])
def test_the_chain_cut_into_two_launches_and_continued_raw_is_the_whole(with_fracs):
    """voices [0, 20) raw, then [20, 37) in place through init: what the tiles of a piece do"""
    import torch
    ctx = stereo_context("union_window")
    rows, onsets, lengths, gains, pans, _, fracs = sc.planted(37, NT)
    f = fracs if with_fracs else None
    _, pointers = device_rows(37)
    samples, channels = [r.shape[1] for r in rows], [r.shape[0] for r in rows]
    d_out = torch.zeros(2 * NT, dtype=torch.float32, device="cuda")
    d_gains = torch.from_numpy(np.array(gains)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.score_rows_stereo(pointers[:20], samples[:20], channels[:20], onsets[:20], pans[:20], NT, d_out.data_ptr(), lengths[:20], d_gains.data_ptr(), None, True,
                          fracs=None if f is None else f[:20], stream=stream)
    ctx.score_rows_stereo(pointers[20:], samples[20:], channels[20:], onsets[20:], pans[20:], NT, d_out.data_ptr(), lengths[20:], d_gains.data_ptr() + 4 * 20, d_out.data_ptr(), False,
                          fracs=None if f is None else f[20:], stream=stream)
    torch.cuda.synchronize()
    kernel, plan, upload = ctx.score_last_ms()  # (dusp_score_last_ms reports the stereo call)
    assert 0 < kernel < 1000 and 0 <= plan < 1000 and 0 < upload < 1000
    same(d_out.cpu().numpy().reshape(2, NT), expected(37, "in_turn", True, True, False, False, with_fracs), "two launches")


@pytest.mark.parametrize("with_fracs", [False, True], ids=["whole", "fracs"])
@pytest.mark.parametrize("n", [9, 37])
def test_lists_of_one_kind_give_the_bits_of_the_existing_calls(n, with_fracs):
    """all voices mono and panned: dusp_score_rows_pan_device's (with fractions: dusp_score_rows_frac_device's) bits; all voices of two
    channels: dusp_score_rows_device's"""
    import torch
    ctx = stereo_context("union_window")
    stream = torch.cuda.current_stream().cuda_stream
    for kinds in (sc.PANNED, sc.TWO):
        rows, onsets, lengths, gains, pans, init, fracs = sc.planted(n, NT, kinds)
        f = fracs if with_fracs else None
        _, pointers = device_rows(n, kinds)
        samples = [r.shape[1] for r in rows]
        d_gains = torch.from_numpy(np.array(gains)).cuda()
        d_init = torch.from_numpy(np.array(init).reshape(-1)).cuda()
        d_old, d_new = (torch.full((2 * NT,), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        for raw in (True, False):
            if kinds == sc.PANNED:
                ctx.score_rows_frac(pointers, samples, 1, onsets, f, NT, d_old.data_ptr(), lengths, d_gains.data_ptr(), d_init.data_ptr(), raw, pans=pans, stream=stream)
            else:
                ctx.score_rows_frac(pointers, samples, 2, onsets, f, NT, d_old.data_ptr(), lengths, d_gains.data_ptr(), d_init.data_ptr(), raw, stream=stream)
            ctx.score_rows_stereo(pointers, samples, [r.shape[0] for r in rows], onsets, pans, NT, d_new.data_ptr(), lengths, d_gains.data_ptr(), d_init.data_ptr(), raw, fracs=f,
                                  stream=stream)
            torch.cuda.synchronize()
            old, new = d_old.cpu().numpy().reshape(2, NT), d_new.cpu().numpy().reshape(2, NT)
            same(new, old, (kinds, raw))
            same(new, expected(n, kinds, True, True, True, raw, with_fracs), (kinds, raw, "contract"))


def test_no_voices_rows_of_two_channels_of_no_and_one_sample_and_a_first_voice_without_a_row():
    import torch
    ctx = render.context(48000)
    stream = torch.cuda.current_stream().cuda_stream
    init = np.array([[1.0, -0.0, np.nan, 0.0, -2.5, np.inf, 1e-45, 0.0], [-0.0, 3.0, 0.0, np.nan, -np.inf, 2.0, -1e-45, 0.0]], dtype=np.float32)
    d_buf = torch.from_numpy(init.reshape(-1).copy()).cuda()
    d_out = torch.full((16,), 9.0, dtype=torch.float32, device="cuda")
    ctx.score_rows_stereo([], [], [], [], None, 8, d_out.data_ptr(), d_init=d_buf.data_ptr(), raw=True, stream=stream)
    torch.cuda.synchronize()
    same(d_out.cpu().numpy().reshape(2, 8), init, "raw: a copy of both channels")
    ctx.score_rows_stereo([], [], [], [], [], 8, d_out.data_ptr(), d_init=d_buf.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    same(d_out.cpu().numpy().reshape(2, 8), score_chain_rows_stereo([], [], None, 8, init=init), "`|| 0` of both channels")
    # voice 0 is a two-channel row of NO samples (no row at all: the padded entries name it), voice 1 one of ONE sample, voice 2 mono
    rows, onsets, pans = sc.edge_rows()
    one = torch.tensor([1.5, -2.5], dtype=torch.float32, device="cuda")
    three = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float32, device="cuda")
    for fracs in (None, [0.0, 0.5, 0.25]):
        ctx.score_rows_stereo([None, one.data_ptr(), three.data_ptr()], [0, 1, 3], [2, 2, 1], onsets, pans, 8, d_out.data_ptr(), fracs=fracs, stream=stream)
        torch.cuda.synchronize()
        same(d_out.cpu().numpy().reshape(2, 8), score_chain_rows_stereo(rows, onsets, pans, 8, fracs=fracs), "edge rows")
    assert d_out.cpu().numpy().reshape(2, 8)[:, 4].tolist() == [0.75 + 0.25 * 1.0 + 0.75 * 2.0, -1.25 + 0.25 * 1.0 + 0.75 * 2.0]
    # a panned voice with pan 0 and a compensation of 2 beside an unplaced one: the mono samples on both channels
    ctx.score_rows_stereo([three.data_ptr(), three.data_ptr()], [3, 3], [1, 1], [1, 4], [0.0, None], 8, d_out.data_ptr(), comp=[2.0, 1.0], stream=stream)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tolist() == [0, 1, 2, 3, 1, 2, 3, 0] * 2


# ---- dusp_render_host_score_parts_stereo, render_piece(..., stereo=True) --------------------------------------------------------------------

def piece_args(n, with_fracs=False):
    rate = sv.SAMPLE_RATE
    onsets, fracs, gains = sc.layout(n, with_fracs)
    return onsets, fracs, gains, (sv.NV + 0.5) / rate, (sv.NT + 0.5) / rate


@functools.lru_cache(maxsize=None)
def oracle_piece(n, order, with_gains, with_fracs, oracle):
    """the oracle's render of the piece as ONE circuit (tests/test_stereo_host.py anchors the numpy contract to it)"""
    d.configure(sv.SAMPLE_RATE)
    onsets, fracs, gains, _, _ = piece_args(n, with_fracs)
    circuit = sc.as_one_stereo_circuit(sc.voices_for(n, order), onsets, sc.stereo_pans(n, order), gains if with_gains else None, fracs)
    want = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
    want.setflags(write=False)
    return want


def test_a_mono_voice_beside_a_two_channel_voice_renders_only_as_a_stereo_piece(oracle):
    """without the keyword the piece is refused, as it always was; with it, it is the oracle's one circuit"""
    d.configure(sv.SAMPLE_RATE)
    voices = lambda: [sc.voice(0, sc.MONO), sc.voice(1, sc.TWO)]
    onsets, dur, voice_dur = [0, 40], (sv.NT + 0.5) / sv.SAMPLE_RATE, (sv.NV + 0.5) / sv.SAMPLE_RATE
    with pytest.raises(descriptor.DuspError, match="the voices of a piece must have one number of output channels: part 1 has 2, part 0 has 1"):
        d.render_piece(voices(), onsets, voice_dur, dur)
    got = np.stack(d.render_piece(voices(), onsets, voice_dur, dur, stereo=True))
    want = np.asarray(oracle.render(descriptor.extract(sc.as_one_stereo_circuit(voices(), onsets, [None, None])).words, sv.NT), dtype=np.float32)
    assert want.shape == (2, sv.NT) and np.abs(want).max() > 0 and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("with_fracs", [False, True], ids=["whole", "fracs"])
@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("n", [2, 13, 37])
def test_render_piece_stereo_is_the_oracles_one_circuit(n, order, with_fracs, oracle):
    """three structures — the panned mono voice, the plain mono voice, the voice of two channels — in one tile and in many"""
    with_gains = n != 13
    want = oracle_piece(n, order, with_gains, with_fracs, oracle)
    assert want.shape == (2, sv.NT)
    onsets, fracs, gains, voice_dur, dur = piece_args(n, with_fracs)
    g = gains if with_gains else None
    pans = [None if np.isnan(p) else float(p) for p in sc.stereo_pans(n, order)]
    d.configure(sv.SAMPLE_RATE)
    # tiles: the default (one), and 7000 bytes — a mono row has 3092 bytes, one of two channels 6184: two mono voices or one wide voice a tile
    results = {}
    for tile_bytes in (0, 7000) if n > 2 else (0, 1):
        got = d.render_piece(sc.voices_for(n, order), onsets, voice_dur, dur, None, g, tile_bytes=tile_bytes, pans=pans, fracs=fracs, stereo=True)
        assert got.sampleRate == sv.SAMPLE_RATE and len(got) == 2 and got[0].shape == (sv.NT,)
        results[tile_bytes] = np.stack(got)
    a, b = results.values()
    print("n %d %s fracs %s: %d samples differ between the tilings, %d from the oracle" % (n, order, with_fracs, int((bits(a) != bits(b)).sum()), int((bits(a) != bits(want)).sum())))
    assert np.array_equal(bits(a), bits(b)), "the two tilings differ"
    for tile_bytes, got in results.items():
        assert np.array_equal(bits(got), bits(want)), (tile_bytes, "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0))))


def test_render_score_stereo_and_pieces_of_one_kind():
    d.configure(sv.SAMPLE_RATE)
    n = 5
    onsets, lengths, gains = sv.layout(n)
    dur, voice_dur = (sv.NT + 0.5) / sv.SAMPLE_RATE, (sv.NV + 0.5) / sv.SAMPLE_RATE
    wide = lambda: [sc.voice(k, sc.TWO) for k in range(n)]
    mono = lambda: [sv.voice(k) for k in range(n)]
    # two-channel voices: the plain score's bits; panned mono voices: the panned score's; without the keyword nothing has changed
    want = np.stack(d.render_score(wide(), onsets, voice_dur, dur, lengths, gains))
    got = np.stack(d.render_score(wide(), onsets, voice_dur, dur, lengths, gains, stereo=True))
    assert want.shape == (2, sv.NT) and np.abs(want).max() > 0 and np.array_equal(bits(got), bits(want))
    pans = [-1, 0.25, 0, 1, -0.5]
    want = np.stack(d.render_score(mono(), onsets, voice_dur, dur, lengths, gains, pans=pans))
    got = np.stack(d.render_score(mono(), onsets, voice_dur, dur, lengths, gains, pans=pans, stereo=True))
    assert np.array_equal(bits(got), bits(want))
    # mono voices that are not placed: the mono score on both channels
    want = np.stack(d.render_score(mono(), onsets, voice_dur, dur, lengths, gains))
    got = np.stack(d.render_score(mono(), onsets, voice_dur, dur, lengths, gains, stereo=True))
    assert want.shape == (1, sv.NT) and got.shape == (2, sv.NT) and np.array_equal(bits(got[0:1]), bits(want)) and np.array_equal(bits(got[1:2]), bits(want))
    assert len(d.render_score(mono(), onsets, voice_dur, 0, stereo=True)) == 0


def test_render_piece_pcm_and_wav_stereo():
    """s16 / s24 / f32 frames and the peak of the stereo piece: wav.encode_frames over the f32 result, two channels a frame; the file."""
    n, order = 13, "in_turn"
    rate = sv.SAMPLE_RATE
    d.configure(rate)
    onsets, _, gains, voice_dur, dur = piece_args(n)
    pans = sc.stereo_pans(n, order)
    voices = lambda: sc.voices_for(n, order)
    piece_f32 = np.stack(d.render_piece(voices(), onsets, voice_dur, dur, None, gains, tile_bytes=20000, pans=pans, stereo=True))
    peak_want = np.float32(np.abs(piece_f32).max())
    assert piece_f32.shape == (2, sv.NT) and peak_want > 1.0  # (normalise = 1 has something to shrink)
    for depth, normalise in ((16, 0), (16, 1), (24, 2), (32, 0)):
        res = d.render_piece_pcm(voices(), onsets, voice_dur, dur, depth, normalise, None, gains, tile_bytes=20000, pans=pans, stereo=True)
        want, want_peak = wav.encode_frames(piece_f32, depth, normalise)
        assert res.data.dtype == want.dtype and res.data.shape == want.shape and res.bitDepth == depth and res.numberOfChannels == 2
        assert np.array_equal(res.data.view(np.uint8), want.view(np.uint8)), (depth, normalise)
        assert np.float32(res.peak).view(np.uint32) == np.float32(want_peak).view(np.uint32) == peak_want.view(np.uint32)
    file = d.render_piece_wav(voices(), onsets, voice_dur, dur, 16, 0, None, gains, pans=pans, stereo=True)
    assert file == wav.encode_wav([c for c in piece_f32], rate, 16) and file[:4] == b"RIFF"
    score_file = d.render_score_wav([sc.voice(k, sc.TWO) for k in range(3)], [0, 10, 20], voice_dur, dur, 16, 0, stereo=True)
    score_f32 = np.stack(d.render_score([sc.voice(k, sc.TWO) for k in range(3)], [0, 10, 20], voice_dur, dur, stereo=True))
    assert score_file == wav.encode_wav([c for c in score_f32], rate, 16)


def test_refusals_on_a_live_context():
    import torch
    d.configure(sv.SAMPLE_RATE)
    ctx = knob_context(sv.SAMPLE_RATE, DUSP_WAVE_JIT=2)
    unify = lambda voices: descriptor.unify([descriptor.extract(v) for v in voices])
    mono, wide_uni, three_uni = unify([sv.voice(k) for k in range(2)]), unify([sc.voice(k, sc.TWO) for k in range(2)]), unify([d.Multiply(sv.voice(k), [0.5, 0.25, 0.125]) for k in range(2)])
    a, wide, three = ctx.build(mono.words), ctx.build(wide_uni.words), ctx.build(three_uni.words)
    L, nan = ctx._L, float("nan")
    try:
        assert three.n_out_channels == 3
        # the binder's checks, in front of the library's
        with pytest.raises(ValueError, match="a two-channel voice is not panned: the pan of voice 1 must be NaN"):
            ctx.render_score_parts([(a, 64, 2, mono.params), (wide, 64, 2, wide_uni.params)], [0, 1, 0, 1], [0, 1, 2, 3], 128, pans=[0, 0, 0, None], stereo=True)
        with pytest.raises(ValueError, match="a voice of a stereo piece has one or two channels: voice 1 has 3"):
            ctx.render_score_parts([(a, 64, 2, mono.params), (three, 64, 2, three_uni.params)], [0, 1, 0, 1], [0, 1, 2, 3], 128, stereo=True)
        with pytest.raises(ValueError, match="places and stereo do not go together"):
            ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, taps=(np.zeros((2, 2)), np.ones((2, 2))), stereo=True)
        # the library's own, behind the binder's: the C calls
        buf = torch.zeros(1024, dtype=torch.float32, device="cuda")
        rows = np.array([buf.data_ptr(), buf.data_ptr()], dtype=np.uint64)
        samples, onsets = np.array([8, 8], dtype=np.uint32), np.array([0, 1], dtype=np.int64)
        f32, u32 = lambda *v: np.array(v, dtype=np.float32), lambda *v: np.array(v, dtype=np.uint32)

        def device(channels, pans, fracs=None, n_total=16, out=buf.data_ptr() + 2048, lengths=None, row_ptrs=rows):
            return L.dusp_score_rows_stereo_device(ctx._h, row_ptrs.ctypes.data, samples.ctypes.data, None if channels is None else channels.ctypes.data, 2, onsets.ctypes.data,
                                                   None if fracs is None else fracs.ctypes.data, None if lengths is None else lengths.ctypes.data, None,
                                                   None if pans is None else pans.ctypes.data, None, n_total, None, 0, out, None)
        for call, needle in [
            (lambda: device(u32(1, 2), f32(0.5, 0.0)), b"dusp_score_rows_stereo_device: voice 1 has two channels and a pan: a two-channel voice is not panned"),
            (lambda: device(u32(1, 3), f32(0.5, nan)), b"dusp_score_rows_stereo_device: voice 1 has 3 channels: a voice of a stereo piece has one or two"),
            (lambda: device(u32(0, 1), f32(nan, nan)), b"voice 0 has 0 channels"),
            (lambda: device(u32(1, 2), None), b"dusp_score_rows_stereo_device: h_pans is NULL"),
            (lambda: device(None, f32(nan, nan)), b"dusp_score_rows_stereo_device: h_row_channels is NULL"),
            (lambda: device(u32(1, 2), f32(np.inf, nan)), b"dusp_score_rows_stereo_device: the pan of voice 0 is not finite"),
            (lambda: device(u32(1, 2), f32(nan, nan), fracs=np.array([0.0, 1.0])), b"dusp_score_rows_stereo_device: the fraction of voice 1 is outside [0, 1)"),
            (lambda: device(u32(1, 2), f32(nan, nan), n_total=(1 << 30) + 1), b"channels x timeline samples must not exceed 2^31"),
            (lambda: device(u32(1, 2), f32(nan, nan), row_ptrs=np.array([buf.data_ptr(), 0], dtype=np.uint64)), b"dusp_score_rows_stereo_device: the row of voice 1 is NULL"),
            (lambda: device(u32(1, 2), f32(nan, nan), lengths=np.array([8, 9], dtype=np.int64)), b"length of voice 1 is 9"),
            (lambda: device(u32(1, 2), f32(nan, nan), out=buf.data_ptr() + 2050), b"4-byte aligned"),
        ]:
            assert call() == -1 and needle in L.dusp_last_error(ctx._h), (needle, L.dusp_last_error(ctx._h))
        out = np.zeros((2, 128), dtype=np.float32)
        part = lambda prog, uni: runtime.ScorePart(prog._h, 2, 64, uni.params.ctypes.data if uni.params is not None else None)
        part_of, onsets4 = np.array([0, 1, 0, 1], dtype=np.uint32), np.arange(4, dtype=np.int64)

        def host(table, pans, fracs=None):
            return L.dusp_render_host_score_parts_stereo(table, 2, 4, part_of.ctypes.data, onsets4.ctypes.data, None if fracs is None else fracs.ctypes.data, None, None,
                                                         None if pans is None else pans.ctypes.data, None, 128, 0, 0, 0, out.ctypes.data, None)
        mixed = (runtime.ScorePart * 2)(part(a, mono), part(wide, wide_uni))
        wider = (runtime.ScorePart * 2)(part(a, mono), part(three, three_uni))
        for call, needle in [
            (lambda: host(mixed, f32(0.5, nan, nan, 0.25)), b"dusp_render_host_score_parts_stereo: voice 3 has two channels and a pan: a two-channel voice is not panned"),
            (lambda: host(wider, f32(nan, nan, nan, nan)), b"dusp_render_host_score_parts_stereo: part 1 has 3 output channels: a voice of a stereo piece has one or two"),
            (lambda: host(mixed, None), b"dusp_render_host_score_parts_stereo: h_pans is NULL"),
            (lambda: host(mixed, f32(-np.inf, nan, nan, nan)), b"dusp_render_host_score_parts_stereo: the pan of voice 0 is not finite"),
            (lambda: host(mixed, f32(nan, nan, nan, nan), np.array([0, 0, -0.5, 0])), b"dusp_render_host_score_parts_stereo: the fraction of voice 2 is outside [0, 1)"),
        ]:
            assert call() == -1 and needle in L.dusp_last_error(ctx._h), (needle, L.dusp_last_error(ctx._h))
        assert not buf.cpu().numpy().any() and not out.any()  # (nothing ran)
        # the existing calls refuse what they refused: parts of different channel counts, and a NaN pan
        with pytest.raises(runtime.DuspHipError, match="all parts of a piece have the same number"):
            ctx.render_score_parts([(a, 64, 2, mono.params), (wide, 64, 2, wide_uni.params)], [0, 1, 0, 1], [0, 1, 2, 3], 128)
        with pytest.raises(ValueError, match="the pan of voice 1 is not finite"):
            ctx.render_score_parts([(a, 64, 2, mono.params)], [0, 0], [0, 1], 128, pans=[0, nan])
        # and the mixed piece renders on this context
        assert host(mixed, f32(0.5, nan, nan, nan)) == 0 and out.any()
        assert ctx.render_score_parts([(a, 64, 2, mono.params), (wide, 64, 2, wide_uni.params)], [0, 1, 0, 1], [0, 1, 2, 3], 128, pans=[-1, None, None, None], stereo=True).shape == (2, 128)
    finally:
        a.close()
        wide.close()
        three.close()
