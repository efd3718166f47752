"""Stems on the device (dusp_render_host_score_piece_stems, dusp_score_stems_mix_device, dusp_score_stems_return_device,
dusp_peak_common_device).  The expected value is the contract over the CPU oracle's renders (stem_cases.expected:
track_cases.expected's pieces, mix.track_terms, mix.stems).  Bit for bit; a Filter track is held within 1e-5 of the expected signal's
largest magnitude, the figure tests/test_gpu_tracks.py uses.  Every call's peaks are held to wav.peak of the expected signals.
tests/test_stems_host.py anchors the contract.

Measured on an MI355X: every signal of every case below came out bit for bit, the Filter tracks' too (each test prints its figures)."""
import ctypes
import functools

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
import send_cases as sc
import stem_cases as stc
import stereo_cases as stereo
import track_cases as tc
from frac_cases import layout as frac_layout
from pan_cases import pans_for
from dusp_amd import descriptor, mix, render, runtime, wav
from test_piece_host import NV_SAW, bits, interleaved_voice, oracle_rows, same

pytestmark = pytest.mark.gpu

RATE = sv.SAMPLE_RATE
ENGINES = {"auto": runtime.ENGINE_AUTO, "chunk": runtime.ENGINE_CHUNK, "wave": runtime.ENGINE_WAVE}
N = 13
DUR, VOICE_DUR = (sv.NT + 0.5) / RATE, (sv.NV + 0.5) / RATE


def voices(n=N):
    return [interleaved_voice(k) for k in range(n)]


def mono(n=N):
    return [sv.voice(k) for k in range(n)]


def durations(n=N):
    return [((sv.NV if k % 2 == 0 else NV_SAW) + 0.5) / RATE for k in range(n)]


def stacked(got):
    """a Stems of ChannelData -> float32 [S + 1, channels, n_total], in the order of its names"""
    assert isinstance(got, render.Stems)
    assert all(a is b for a, b in zip([got[name] for name in got.names], [got.direct] + got.tracks + got.buses + [got.mix]))
    return np.stack([np.stack(got[name]) for name in got.names])


def held(name, got, want, filters=()):
    """every signal bit for bit (the Filter tracks' stems, and what hears them: within 1e-5 of the expected signal's largest magnitude),
    every peak wav.peak of the expected signal, and the common peak the largest of them"""
    stack = stacked(got)
    assert stack.dtype == np.float32 and stack.shape == want.shape and got.names == mix.stem_names(len(got.tracks), len(got.buses))
    for s, signal in enumerate(got.names):
        differ = int((bits(stack[s]) != bits(want[s])).sum())
        err, top = float(np.abs(stack[s].astype(np.float64) - want[s]).max()), float(np.abs(want[s]).max())
        print("%s, %s: %d samples differ in bits, max |err| %.3g, max |want| %.3g, peak %r" % (name, signal, differ, err, top, got.peaks[signal]))
        if signal in filters:
            assert err <= 1e-5 * top, (signal, err)
            assert abs(float(got.peaks[signal]) - top) <= 1e-5 * top
        else:
            assert differ == 0, "%s: first differing sample %d" % (signal, int(np.argmax((bits(stack[s]) != bits(want[s])).any(axis=0))))
            assert bits(np.float32(got.peaks[signal])) == bits(wav.peak(want[s])), signal
    assert bits(got.peak) == bits(wav.common_peak(np.array([got.peaks[s] for s in got.names], dtype=np.float32)))
    return stack


@functools.lru_cache(maxsize=None)
def piece_expected(names, with_faders, oracle, buses=(), master=None, n_of=None):
    """the two-instrument piece with the named tracks (None: a track without a circuit), once for the tests that share it"""
    onsets, _, gains = sv.layout(N)
    fxs = [None if name is None else tc.TRACKS[name] for name in names]
    want = stc.expected(oracle, list(oracle_rows(N, oracle)), onsets, sv.NT, fxs, tc.track_of(N, n_of or len(names)), 1, tc.faders(len(names)) if with_faders else None, gains=gains,
                        buses=[tc.TRACKS[b] for b in buses], track_sends=tc.levels(len(buses), len(names)) if buses else None, master=None if master is None else tc.TRACKS[master])
    want.setflags(write=False)
    return want


def piece(names, with_faders=False, n_of=None, **kw):
    onsets, _, gains = sv.layout(N)
    d.configure(RATE)
    fxs = [None if name is None else tc.TRACKS[name] for name in names]
    return d.render_piece(voices(), onsets, durations(), DUR, None, gains, tracks=fxs, track_of=tc.track_of(N, n_of or len(names)),
                          faders=tc.faders(len(names)) if with_faders else None, **kw)


@pytest.mark.parametrize("engine", list(ENGINES))
def test_clip_and_echo_tracks_with_direct_voices_on_every_engine(engine, oracle):
    want = piece_expected(("clip", "echo"), False, oracle)
    got = piece(("clip", "echo"), engine=ENGINES[engine], stems=True)
    assert got.mix.sampleRate == RATE and got.names == ["direct", "track0", "track1", "mix"]
    stack = held("clip+echo, " + engine, got, want)
    assert np.array_equal(bits(mix.stems_sum(stack)), bits(stack[-1])), "the delivered stems do not add up to the delivered mix"
    assert all(stack[s].any() for s in range(4)) and np.array_equal(bits(stack[-1]), bits(np.stack(piece(("clip", "echo"), engine=ENGINES[engine])))), "the mix is not the call's without stems"


def test_a_fader_group_a_track_with_no_voices_and_a_filter_track(oracle):
    names = ("clip", None, "echo")
    want = piece_expected(names, True, oracle, n_of=2)
    stack = held("clip, fader group, silent echo", piece(names, True, n_of=2, stems=True), want)
    assert not stack[3].any() and stack[2].any(), "the echo without voices is a zero stem; the fader group is heard"
    names = ("lowpass", "lowpass", "clip")
    held("filter x2 + clip", piece(names, True, stems=True), piece_expected(names, True, oracle), filters=("track0", "track1", "mix"))


def test_two_buses_fed_by_the_tracks_and_a_master_behind_them(oracle):
    names, buses = ("clip", "echo", None), ("echo", "comb")
    want = piece_expected(names, True, oracle, buses, "allpass")
    got = piece(names, True, buses=[mc.echo, mc.comb], track_sends=tc.levels(2, 3), master=mc.allpass, stems=True)
    assert got.names == ["direct", "track0", "track1", "track2", "bus0", "bus1", "mix"]
    stack = held("tracks, buses and a master", got, want)
    no_master = piece_expected(names, True, oracle, buses)
    assert np.array_equal(bits(want[:-1]), bits(no_master[:-1])) and (bits(stack[-1]) != bits(no_master[-1])).sum() > 1000, "the stems are in front of the master, the mix behind it"
    assert np.array_equal(bits(stack[-1]), bits(np.stack(piece(names, True, buses=[mc.echo, mc.comb], track_sends=tc.levels(2, 3), master=mc.allpass))))
    held("tracks and buses", piece(names, True, buses=[mc.echo, mc.comb], track_sends=tc.levels(2, 3), stems=True), no_master)


@pytest.mark.parametrize("panned", [False, True], ids=["plain", "pans"])
def test_per_note_sends_without_tracks(panned, oracle):
    onsets, _, gains = sv.layout(N)
    d.configure(RATE)
    levels = sc.levels(N, 2)
    if panned:
        rows, make, kw, ckw, channels, dur = tc.oracle_voice_rows(oracle, mono(), [sv.NV] * N), mono, dict(pans=pans_for(N)), dict(pans=pans_for(N)), 2, VOICE_DUR
    else:
        rows, make, kw, ckw, channels, dur = list(oracle_rows(N, oracle)), voices, {}, {}, 1, durations()
    for master in (None, mc.allpass):
        want = stc.expected(oracle, rows, onsets, sv.NT, channels=channels, gains=gains, buses=[mc.echo, mc.comb], sends=levels, master=master, **ckw)
        got = d.render_piece(make(), onsets, dur, DUR, None, gains, buses=[mc.echo, mc.comb], sends=levels, master=master, stems=True, **kw)
        assert got.names == ["direct", "bus0", "bus1", "mix"] and len(got.mix) == channels
        stack = held("sends, master %s" % (master is not None), got, want)
        assert np.array_equal(bits(stack[-1]), bits(np.stack(d.render_piece(make(), onsets, dur, DUR, None, gains, buses=[mc.echo, mc.comb], sends=levels, master=master, **kw))))


def test_neither_tracks_nor_buses(oracle):
    onsets, _, gains = sv.layout(N)
    d.configure(RATE)
    want = stc.expected(oracle, list(oracle_rows(N, oracle)), onsets, sv.NT, gains=gains)
    stack = held("one timeline", d.render_piece(voices(), onsets, durations(), DUR, None, gains, stems=True), want)
    assert stack.shape[0] == 2 and np.array_equal(bits(stack[0]), bits(stack[1])), "S = 1: direct is the mix"
    assert np.array_equal(bits(stack[1]), bits(np.stack(d.render_piece(voices(), onsets, durations(), DUR, None, gains))))
    want = stc.expected(oracle, list(oracle_rows(N, oracle)), onsets, sv.NT, gains=gains, master=mc.echo)
    stack = held("one timeline and a master", d.render_piece(voices(), onsets, durations(), DUR, None, gains, master=mc.echo, stems=True), want)
    assert (bits(stack[0]) != bits(stack[1])).sum() > 1000


def placements():
    """name -> (voices, onsets, gains, the call's keywords, the contract's keywords, the timeline's channels)"""
    onsets, _, gains = sv.layout(N)
    frac_onsets, fracs, frac_gains = frac_layout(N)
    places = np.random.RandomState(5).uniform(-3, 3, (N, 2))
    speakers = [[-1.5, 0], [1.5, 0], [0, 2]]
    return {
        "fracs": (mono, frac_onsets, frac_gains, dict(fracs=fracs), dict(fracs=fracs), 1),
        "places": (mono, onsets, gains, dict(places=places, speakers=speakers), dict(taps=mix.space_taps(places, speakers, sample_rate=RATE)), 3),
        "stereo": (lambda: stereo.voices_for(N, "in_turn"), onsets, gains, dict(pans=stereo.stereo_pans(N, "in_turn"), stereo=True), dict(pans=stereo.stereo_pans(N, "in_turn"), stereo=True), 2),
    }


@pytest.mark.parametrize("placement", ["fracs", "places", "stereo"])
def test_one_track_behind_a_placement(placement, oracle):
    d.configure(RATE)
    make, onsets, gains, kw, contract_kw, channels = placements()[placement]
    rows = tc.oracle_voice_rows(oracle, make(), [sv.NV] * N)
    of, f = tc.track_of(N, 1), tc.faders(1)
    want = stc.expected(oracle, rows, onsets, sv.NT, [mc.clip], of, channels, f, gains=gains, **contract_kw)
    got = d.render_piece(make(), onsets, VOICE_DUR, DUR, None, gains, tracks=[mc.clip], track_of=of, faders=f, stems=True, **kw)
    assert len(got.mix) == len(got.direct) == len(got.tracks[0]) == channels
    stack = held("clip, " + placement, got, want)
    assert stack[0].any() and stack[1].any()


def test_small_tiles_repetition_and_a_call_without_stems_afterwards(oracle):
    names = ("clip", "echo")
    want = piece_expected(names, True, oracle)
    # 9000 bytes: two or three voices of 3092 and 4124 bytes a tile, at least five tiles; 1: one voice a tile
    for tile_bytes in (9000, 1, 0, 0):
        held("tile_bytes %d" % tile_bytes, piece(names, True, tile_bytes=tile_bytes, stems=True), want)
    assert np.array_equal(bits(np.stack(piece(names, True))), bits(want[-1])), "a call without stems is not what it was"
    # ONE context and ONE set of programs reused from call to call, with lengths: stems, none, stems with buses, stems
    ctx = runtime.Context(-1, RATE)
    uni = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(N)])
    t, bus = mc.unified_master(mc.echo, 1), mc.unified_master(mc.comb, 1)
    part, track, comb = ctx.build(uni.words), ctx.build(t.words), ctx.build(bus.words)
    onsets, lengths, gains = sv.layout(N)
    of = tc.track_of(N, 2)
    try:
        run = lambda **kw: ctx.render_score_parts([(part, sv.NV, N, uni.params)], [0] * N, onsets, sv.NT, lengths, gains, **kw)
        with_tracks = dict(tracks=dict(n_tracks=2, track_of=of, programs=[(track, [1], t.params)]))
        rows = [np.asarray(r, dtype=np.float32) for r in oracle.render_instances(uni.words, sv.NV, uni.params, N, range(N))]
        want = stc.expected(oracle, rows, onsets, sv.NT, [None, mc.echo], of, 1, None, lengths, gains)
        first, peaks = run(stems=True, **with_tracks)
        assert np.array_equal(bits(first), bits(want)) and np.array_equal(bits(peaks), bits(np.array([wav.peak(x) for x in want])))
        assert np.array_equal(bits(run(**with_tracks)), bits(want[-1]))
        wide = dict(tracks=dict(n_tracks=2, track_of=of, programs=[(track, [1], t.params)], track_sends=tc.levels(1, 2)), buses=[(comb, bus.params)])
        want_wide = stc.expected(oracle, rows, onsets, sv.NT, [None, mc.echo], of, 1, None, lengths, gains, buses=[mc.comb], track_sends=tc.levels(1, 2))
        assert np.array_equal(bits(run(stems=True, tile_bytes=7000, **wide)[0]), bits(want_wide)), "a larger block after a smaller one"
        again, again_peaks = run(stems=True, **with_tracks)
        assert np.array_equal(bits(again), bits(first)) and np.array_equal(bits(again_peaks), bits(peaks)), "the second call differs"
    finally:
        for p in (part, track, comb):
            p.close()
        ctx.close()


# ---- one gain, every format ---------------------------------------------------------------------------------------------------------------

M = 12  # voices 2j and 2j + 1 are one voice at one onset, the second a hundredth louder, on two fader groups at faders +1 and -1


def loud_case():
    onsets = np.repeat(sv.layout(M)[0][::2], 2)
    gains = np.repeat(np.array([1.9, 1.2, 1.5, 1.7, 1.3, 1.8], dtype=np.float32), 2)  # (a voice peaks near 1: every stem clips)
    gains[1::2] *= np.float32(1.01)
    of, f = stc.opposed(M)
    return [sv.voice(k // 2) for k in range(M)], onsets, gains, of, f


def test_frames_of_every_format_under_the_common_gain_where_a_stem_is_louder_than_the_mix(oracle):
    d.configure(RATE)
    make, onsets, gains, of, f = loud_case()
    rows = tc.oracle_voice_rows(oracle, make, [sv.NV] * M)
    want = stc.expected(oracle, rows, onsets, sv.NT, [None, None], of, 1, f, gains=gains)
    own = np.array([wav.peak(x) for x in want], dtype=np.float32)
    assert own[1] > 1.0 and own[2] > 1.0 and own[3] < 0.05 * own[1] and own[3] > 0, "the stems are louder than the mix, and clip"
    with_tracks = dict(tracks=[None, None], track_of=of, faders=f, stems=True)
    for depth in (16, 24, 32):
        for normalise in (0, 1, 2):
            _, onsets, gains, _, _ = loud_case()
            res = d.render_piece_pcm(loud_case()[0], onsets, VOICE_DUR, DUR, depth, normalise, None, gains, **with_tracks)
            frames, peaks = wav.encode_stems(want, depth, normalise)
            assert isinstance(res, render.Stems) and res.names == ["direct", "track0", "track1", "mix"]
            for s, name in enumerate(res.names):
                one = res[name]
                assert one.data.dtype == frames.dtype and one.data.shape == frames[s].shape and one.bitDepth == depth and one.numberOfChannels == 1
                assert np.array_equal(np.ascontiguousarray(one.data).view(np.uint8), np.ascontiguousarray(frames[s]).view(np.uint8)), (name, depth, normalise)
                assert bits(np.float32(one.peak)) == bits(peaks[s]) == bits(res.peaks[name]) == bits(own[s])
            assert bits(res.peak) == bits(wav.common_peak(own)) and res.gain == wav.gain(wav.common_peak(own), normalise)
            if normalise == 2 and depth == 16:  # (the mix alone would have been blown up to full scale)
                alone = d.render_piece_pcm(loud_case()[0], onsets, VOICE_DUR, DUR, depth, normalise, None, gains, tracks=[None, None], track_of=of, faders=f)
                assert np.abs(alone.data.astype(np.int32)).max() == 32767 and np.abs(res.mix.data.astype(np.int32)).max() < 0.05 * 32767
    files = d.render_piece_wav(loud_case()[0], onsets, VOICE_DUR, DUR, 16, 1, None, gains, **with_tracks)
    frames, _ = wav.encode_stems(want, 16, 1)
    assert files.names == ["direct", "track0", "track1", "mix"] and all(files[name] == wav.encode_wav(frames[s], RATE, 16) for s, name in enumerate(files.names))


def test_render_score_with_stems_is_render_piece_of_one_structure(oracle):
    d.configure(RATE)
    onsets, lengths, gains = sv.layout(N)
    of = tc.track_of(N, 2)
    kw = dict(tracks=[mc.echo, mc.comb], track_of=of, faders=tc.faders(2), stems=True)
    want = stacked(d.render_piece(mono(), onsets, VOICE_DUR, DUR, lengths, gains, **kw))
    got = d.render_score(mono(), onsets, VOICE_DUR, DUR, lengths, gains, **kw)
    rows = tc.oracle_voice_rows(oracle, mono(), [sv.NV] * N)
    stack = held("echo+comb over a score", got, stc.expected(oracle, rows, onsets, sv.NT, [mc.echo, mc.comb], of, 1, tc.faders(2), lengths, gains))
    assert np.array_equal(bits(stack), bits(want))
    plain = d.render_score(mono(), onsets, VOICE_DUR, DUR, lengths, gains, stems=True)  # (a score with stems alone goes the piece's way too)
    assert plain.names == ["direct", "mix"] and np.array_equal(bits(np.stack(plain.mix)), bits(np.stack(d.render_score(mono(), onsets, VOICE_DUR, DUR, lengths, gains))))
    pcm = d.render_score_pcm(mono(), onsets, VOICE_DUR, DUR, 16, 1, lengths, gains, **kw)
    assert np.array_equal(np.stack([pcm[name].data for name in pcm.names]), wav.encode_stems(want, 16, 1)[0])


# ---- the device entries alone -------------------------------------------------------------------------------------------------------------

SENTINEL, GUARD = -12345.678, 64


def planted(n, seed):
    rs = np.random.RandomState(seed)
    a = (rs.standard_normal(n) * 10.0 ** rs.randint(-3, 4, n)).astype(np.float32)
    for j, v in enumerate([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -5e-39, np.finfo(np.float32).max]):
        a[(7 * j + 3 + seed) % n] = v
    return a


def fenced(torch, n, skip):
    """n floats behind GUARD + skip sentinels and in front of GUARD more -> (the tensor, the address of the n floats, their slice)"""
    t = torch.full((GUARD + skip + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return t, t.data_ptr() + 4 * (GUARD + skip), slice(GUARD + skip, GUARD + skip + n)


def untouched(t, inner):
    a = t.cpu().numpy()
    return (a[:inner.start] == np.float32(SENTINEL)).all() and (a[inner.stop:] == np.float32(SENTINEL)).all()


@pytest.mark.parametrize("n", [1, 3, 4, 1027])
def test_the_mix_and_return_entries_alone(n):
    """mix: T = 0, 1 and 8, B = 0 .. 4, with and without faders, raw and not, out of place into buffers off a 16-byte boundary (one float
    a lane) and in place on boundaries (four floats a lane and a tail; with n % 4 != 0 the slots behind the first are off them);
    return: B = 1 .. 4, with and without a direct slot, raw and not, in place and not.  Planted NaN, Inf and -0 in every input."""
    import torch
    ctx = runtime.Context(-1, RATE)
    stream = torch.cuda.current_stream().cuda_stream
    up = lambda a, skip=0: torch.from_numpy(np.concatenate([np.zeros(skip, np.float32), a])).cuda()
    try:
        for T in (0, 1, 8):
            for B in range(5):
                for variant in range(4):
                    with_faders, raw, aligned = (variant & 1) and T > 0, variant >> 1, (variant + B) & 1
                    direct, ys = planted(n, 1 + B), [planted(n, 10 + g + T) for g in range(T)]
                    faders = np.array([0.0, -0.0, 1.0, -0.75, 1e-30, 3e20, 0.6, 2.0][:T], dtype=np.float32) if with_faders else None
                    levels = np.array([[0.0, -0.0, 1.0, -0.5, 1e-30, 3e20, 0.25, 1.5][(b + g) % 8] for b in range(B) for g in range(T)], dtype=np.float32).reshape(B, T) if B else None
                    if T:
                        want, want_feeds = mix.track_mix(direct[None], [y[None] for y in ys], faders, levels)
                    else:  # (no tracks: the mix is the direct timeline and the feeds are +0)
                        want, want_feeds = direct[None].copy(), np.zeros((B, 1, n), dtype=np.float32)
                    want_out = want[0] if raw else mix.bus_return(want, [])[0]
                    want_stems = mix.stems(direct[None], mix.track_terms([y[None] for y in ys], faders), [], want)[:-1, 0]
                    d_ys = [up(y, 0 if aligned else 1) for y in ys]
                    y_ptrs = [t.data_ptr() + (0 if aligned else 4) for t in d_ys]
                    if aligned:  # in place: out is direct
                        d_direct, d_feed, d_stems = up(direct.copy()), torch.zeros(max(B, 1) * n, dtype=torch.float32, device="cuda"), torch.zeros((1 + T) * n, dtype=torch.float32, device="cuda")
                        assert all(p % 16 == 0 for p in [d_direct.data_ptr(), d_feed.data_ptr(), d_stems.data_ptr()] + y_ptrs)
                        ctx.score_stems_mix(d_direct.data_ptr(), y_ptrs, n, d_direct.data_ptr(), d_stems.data_ptr(), faders, levels, d_feed.data_ptr() if B else None, raw=raw, stream=stream)
                        torch.cuda.synchronize()
                        got, got_feeds, got_stems = d_direct.cpu().numpy(), d_feed.cpu().numpy()[:B * n], d_stems.cpu().numpy()
                    else:
                        d_direct = up(direct, 3)
                        (d_out, p_out, in_out), (d_feed, p_feed, in_feed), (d_stems, p_stems, in_stems) = fenced(torch, n, 1), fenced(torch, max(B, 1) * n, 3), fenced(torch, (1 + T) * n, 2)
                        ctx.score_stems_mix(d_direct.data_ptr() + 12, y_ptrs, n, p_out, p_stems, faders, levels, p_feed if B else None, raw=raw, stream=stream)
                        torch.cuda.synchronize()
                        assert untouched(d_out, in_out) and untouched(d_stems, in_stems), "floats beside the output or the stems were written"
                        assert untouched(d_feed, in_feed) if B else (d_feed.cpu().numpy() == np.float32(SENTINEL)).all(), "floats beside the feeds were written"
                        got, got_feeds, got_stems = d_out.cpu().numpy()[in_out], d_feed.cpu().numpy()[in_feed][:B * n], d_stems.cpu().numpy()[in_stems]
                    where = (n, T, B, variant)
                    assert same(got, want_out), where  # (bit patterns, so -0 and +0 too; for NaN, the positions)
                    assert same(got_feeds.reshape(B, n), want_feeds.reshape(B, n)), where
                    assert np.array_equal(bits(got_stems.reshape(1 + T, n)), bits(want_stems)), where
        assert ctx.score_last_ms()[0] > 0
        for B in range(1, 5):
            for variant in range(8):
                with_direct, raw, aligned = variant & 1, (variant >> 1) & 1, (variant >> 2) & 1
                dry, wets = planted(n, 60 + B), [planted(n, 70 + b) for b in range(B)]
                want = mix.bus_return(dry[None], [w[None] for w in wets], raw=bool(raw))[0]
                d_wets = [up(w, 0 if aligned else 1 + b % 3) for b, w in enumerate(wets)]
                w_ptrs = [t.data_ptr() + (0 if aligned else 4 * (1 + b % 3)) for b, t in enumerate(d_wets)]
                d_dry = up(dry.copy(), 0 if aligned else 1)
                p_dry = d_dry.data_ptr() + (0 if aligned else 4)
                (d_out, p_out, in_out), (d_sd, p_sd, in_sd), (d_sb, p_sb, in_sb) = fenced(torch, n, 0 if aligned else 1), fenced(torch, n, 0 if aligned else 3), fenced(torch, B * n, 0 if aligned else 2)
                ctx.score_stems_return(p_dry, w_ptrs, n, p_dry if aligned else p_out, p_sb, p_sd if with_direct else None, raw=raw, stream=stream)  # (aligned: in place)
                torch.cuda.synchronize()
                where = (n, B, variant)
                assert untouched(d_sb, in_sb) and (untouched(d_sd, in_sd) if with_direct else (d_sd.cpu().numpy() == np.float32(SENTINEL)).all()), where
                assert same((d_dry.cpu().numpy() if aligned else d_out.cpu().numpy()[in_out])[-n:], want), where
                assert np.array_equal(bits(d_sb.cpu().numpy()[in_sb].reshape(B, n)), bits(np.stack(wets))), "a bus's slot is a copy of its output"
                if with_direct:
                    assert np.array_equal(bits(d_sd.cpu().numpy()[in_sd]), bits(mix.bus_return(dry[None], [])[0])), where
        assert ctx.score_last_ms()[0] > 0
    finally:
        ctx.close()


def test_the_common_peak_entry_alone_and_the_encoder_behind_it():
    import torch
    ctx = runtime.Context(-1, RATE)
    stream = torch.cuda.current_stream().cuda_stream
    rs = np.random.RandomState(9)
    try:
        for n_peaks in (1, 2, 12, 64, 70):
            for poison in (False, True):
                words = (rs.randint(0, 1 << 31, n_peaks, dtype=np.int64) & 0x7f7fffff).astype(np.uint32)
                if poison:
                    words[n_peaks // 2] = 0x7fc00123  # (a NaN's pattern sorts above every number's, infinity's included)
                d_peaks = torch.from_numpy(words.view(np.float32).copy()).cuda()
                d_common, p_common, inner = fenced(torch, n_peaks, 1)
                ctx.peak_common(d_peaks.data_ptr(), n_peaks, p_common, stream=stream)
                torch.cuda.synchronize()
                assert untouched(d_common, inner)
                got = d_common.cpu().numpy()[inner].view(np.uint32)
                assert (got == words.max()).all() and bits(wav.common_peak(words.view(np.float32)))[0] == words.max(), (n_peaks, poison)
        assert ctx.score_last_ms()[0] > 0
        # peak -> common peak -> encode: three instances under the gain of the loudest, wav.encode_stems' bytes
        stack = (rs.standard_normal((3, 2, 515)) * np.array([0.1, 2.5, 0.7])[:, None, None]).astype(np.float32)
        d_in, d_peaks, d_common = torch.from_numpy(stack).cuda(), torch.zeros(3, dtype=torch.float32, device="cuda"), torch.zeros(3, dtype=torch.float32, device="cuda")
        d_out = torch.zeros(3 * 515 * 2, dtype=torch.int16, device="cuda")
        ctx.peak(d_in.data_ptr(), 3, 2, 515, d_peaks.data_ptr(), stream=stream)
        ctx.peak_common(d_peaks.data_ptr(), 3, d_common.data_ptr(), stream=stream)
        ctx.encode(d_in.data_ptr(), 3, 2, 515, d_out.data_ptr(), "s16", 2, d_common.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        frames, peaks = wav.encode_stems(stack, 16, 2)
        assert np.array_equal(d_out.cpu().numpy().reshape(3, 515, 2), frames) and np.array_equal(bits(d_peaks.cpu().numpy()), bits(peaks))
    finally:
        ctx.close()


# ---- the C entries, through ctypes ------------------------------------------------------------------------------------------------------

def test_the_c_entries_refuse_before_anything_renders():
    d.configure(RATE)
    L = runtime.load()
    ctx = runtime.Context(-1, RATE)
    two = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(2)])
    echo = mc.unified_master([mc.echo_of(300.25)], 1)
    programs = dict(part=ctx.build(two.words), good=ctx.build(echo.words), good2=ctx.build(echo.words))
    parts = (runtime.ScorePart * 1)(runtime.ScorePart(programs["part"]._h, 2, sv.NV, two.params.ctypes.data))
    part_of, onsets = np.zeros(2, dtype=np.uint32), np.array([0, 40], dtype=np.int64)
    out, peaks = np.full((4, 1, 1024), 7, dtype=np.float32), np.full(4, 7, dtype=np.float32)
    who = "dusp_render_host_score_piece_stems: "
    of, which, level = np.array([0, -1], dtype=np.int32), np.array([0], dtype=np.uint32), np.ones((1, 1), dtype=np.float32)
    table = (runtime.ScoreTrackProgram * 1)(runtime.ScoreTrackProgram(programs["good"]._h, 1, which.ctypes.data, None))
    bus_table = (runtime.ScoreMaster * 1)(runtime.ScoreMaster(programs["good2"]._h, None))

    def call(n_signals, tracks=False, buses=False, n_total=1024, h_out=True, stems=True, h_peaks=True):
        routed = runtime.ScoreTracks(1, of.ctypes.data, 1, ctypes.addressof(table), None, level.ctypes.data if buses else None)
        into = runtime.ScoreBuses(1, ctypes.addressof(bus_table), None)
        asked = runtime.ScoreStems(n_signals)
        return L.dusp_render_host_score_piece_stems(parts, 1, 2, part_of.ctypes.data, onsets.ctypes.data, None, None, None, ctypes.addressof(routed) if tracks else None,
                                                    ctypes.addressof(into) if buses else None, None, ctypes.addressof(asked) if stems else None, n_total, 0, 0, 0,
                                                    out.ctypes.data if h_out else None, peaks.ctypes.data if h_peaks else None)

    try:
        for kw, needle in [
            (dict(n_signals=3), "the stems' n_signals is 3, the call delivers 2: the direct mix, 0 tracks, 0 buses and the mix"),
            (dict(n_signals=2, tracks=True), "the stems' n_signals is 2, the call delivers 3: the direct mix, 1 tracks, 0 buses and the mix"),
            (dict(n_signals=3, tracks=True, buses=True), "the stems' n_signals is 3, the call delivers 4: the direct mix, 1 tracks, 1 buses and the mix"),
            (dict(n_signals=0), "the stems' n_signals is 0, the call delivers 2"),
            (dict(n_signals=2, h_out=False), "h_out is NULL: a call with stems delivers its 2 signals there"),
            (dict(n_signals=2, n_total=(1 << 30) + 1), "signals x channels x timeline samples must not exceed 2^31 with stems (2 signals)"),
            (dict(n_signals=3, tracks=True, n_total=(1 << 30)), "signals x channels x timeline samples must not exceed 2^31 with stems (3 signals)"),
        ]:
            assert call(**kw) == -1, needle
            message = L.dusp_last_error(ctx._h).decode()
            assert message.startswith(who) and needle in message, message
            assert (out == 7).all() and (peaks == 7).all(), "a refused call wrote to h_out or h_peaks"
        # the refusals of the entry below it stand, under this entry's name
        routed = runtime.ScoreTracks(9, of.ctypes.data, 0, None, None, None)
        asked = runtime.ScoreStems(11)
        assert L.dusp_render_host_score_piece_stems(parts, 1, 2, part_of.ctypes.data, onsets.ctypes.data, None, None, None, ctypes.addressof(routed), None, None, ctypes.addressof(asked),
                                                    1024, 0, 0, 0, out.ctypes.data, None) == -1
        assert L.dusp_last_error(ctx._h).decode() == mix.TRACKS_COUNT.replace("dusp-hip: ", who) % 9
        # what is asked for rightly renders, h_peaks or not; without stems the entry is dusp_render_host_score_piece_tracks
        assert call(n_signals=4, tracks=True, buses=True) == 0, L.dusp_last_error(ctx._h).decode()
        assert not (out == 7).any() and not (peaks == 7).any() and np.array_equal(bits(peaks), bits(np.array([wav.peak(x) for x in out])))
        whole = out.copy()
        assert call(n_signals=4, tracks=True, buses=True, h_peaks=False) == 0 and np.array_equal(bits(out), bits(whole))
        out[:] = 7
        assert call(n_signals=0, tracks=True, buses=True, stems=False) == 0 and np.array_equal(bits(out[0]), bits(whole[3])) and (out[1:] == 7).all()
        # the device entries' own
        import torch
        buf = torch.zeros(256, dtype=torch.float32, device="cuda")
        p = buf.data_ptr()
        ptrs, none = (ctypes.c_void_p * 8)(*([p] * 8)), (ctypes.c_void_p * 8)()
        one, bad = np.ones((4, 8), dtype=np.float32), np.full((4, 8), np.nan, dtype=np.float32)
        entry = lambda *args: L.dusp_score_stems_mix_device(ctx._h, *args, None)
        for args, needle in [((p, ptrs, 9, None, 0, None, 8, 0, p, None, None, p), "a call has 0 .. 8 tracks, not 9"), ((p, ptrs, 1, None, 5, one.ctypes.data, 8, 0, p, None, p, p), "a call has 0 .. 4 buses, not 5"),
                             ((None, ptrs, 1, None, 0, None, 8, 0, p, None, None, p), "NULL buffer"), ((p, ptrs, 1, None, 0, None, 8, 0, p, None, None, None), "NULL buffer"),
                             ((p, None, 1, None, 0, None, 8, 0, p, None, None, p), "NULL buffer"), ((p, none, 1, None, 0, None, 8, 0, p, None, None, p), "NULL buffer"),
                             ((p, ptrs, 1, None, 1, one.ctypes.data, 8, 0, p, None, None, p), "NULL buffer"), ((p, ptrs, 1, None, 1, None, 8, 0, p, None, p, p), "NULL buffer"),
                             ((p, ptrs, 0, None, 0, None, 0, 0, p, None, None, p), "need 1..2^31 floats"), ((p, ptrs, 1, None, 0, None, 8, 0, p, None, None, p + 2), "4-byte aligned"),
                             ((p, ptrs, 2, bad.ctypes.data, 0, None, 8, 0, p, None, None, p), "the fader of track 0 is not finite"),
                             ((p, ptrs, 2, None, 1, bad.ctypes.data, 8, 0, p, None, p, p), "the level of track 0 into bus 0 is not finite")]:
            assert entry(*args) == -1 and needle in L.dusp_last_error(ctx._h).decode(), needle
        entry = lambda *args: L.dusp_score_stems_return_device(ctx._h, *args, None)
        for args, needle in [((p, ptrs, 0, 8, 0, p, None, p), "a call has 1 .. 4 buses, not 0"), ((p, ptrs, 5, 8, 0, p, None, p), "a call has 1 .. 4 buses, not 5"), ((None, ptrs, 1, 8, 0, p, None, p), "NULL buffer"),
                             ((p, ptrs, 1, 8, 0, p, None, None), "NULL buffer"), ((p, none, 1, 8, 0, p, None, p), "NULL buffer"), ((p, ptrs, 1, 0, 0, p, None, p), "need 1..2^31 floats"),
                             ((p, ptrs, 1, 8, 0, p, p + 2, p), "4-byte aligned")]:
            assert entry(*args) == -1 and needle in L.dusp_last_error(ctx._h).decode(), needle
        entry = lambda *args: L.dusp_peak_common_device(ctx._h, *args, None)
        for args, needle in [((None, 3, p), "NULL buffer"), ((p, 3, None), "NULL buffer"), ((p, 0, p + 64), "need 1..2^24 peaks"), ((p, (1 << 24) + 1, p + 64), "need 1..2^24 peaks"),
                             ((p, 3, p + 2), "4-byte aligned"), ((p, 3, p), "d_common must not be d_peaks")]:
            assert entry(*args) == -1 and needle in L.dusp_last_error(ctx._h).decode(), needle
        torch.cuda.synchronize()
        assert not buf.cpu().numpy().any()  # (nothing ran)
    finally:  # (programs before their contexts, whatever failed)
        for prog in programs.values():
            prog.close()
        ctx.close()
