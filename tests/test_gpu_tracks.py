"""Tracks on the device (dusp_render_host_score_piece_tracks, dusp_score_tracks_mix_device).  The expected value is the
contract over the CPU oracle's renders: the voices' rows from the oracle -> the contract's chain per destination (track_cases.sub_chain:
the placement's own function over the destination's voices) -> every track circuit rendered over its sub-mix by the oracle
(master_cases.oracle_master) -> mix.track_mix -> the buses -> the master.  Bit for bit; a Filter track is held within 1e-5 of the
expected signal's largest magnitude, the figure tests/test_gpu_master.py uses.  tests/test_tracks_host.py anchors the contract."""
import ctypes
import functools

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
import stereo_cases as stc
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
CHANNEL_ECHOES = [mc.echo_of(300.25), mc.echo_of(411.5), mc.echo_of(257.75)]  # a track circuit a channel: one program, the delay its parameter


def voices(n=N):
    return [interleaved_voice(k) for k in range(n)]


def durations(n=N):
    return [((sv.NV if k % 2 == 0 else NV_SAW) + 0.5) / RATE for k in range(n)]


def held(name, got, want, before=None):
    """bit for bit (a Filter track: within 1e-5 of the expected signal's largest magnitude), and the tracks are heard"""
    got = np.stack(got) if not isinstance(got, np.ndarray) else got
    assert got.dtype == np.float32 and got.shape == want.shape
    differ = int((bits(got) != bits(want)).sum())
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: %d samples differ in bits, max |err| %.3g, max |want| %.3g" % (name, differ, err, float(np.abs(want).max())))
    if before is not None:
        assert (bits(want) != bits(before)).any(axis=0).sum() > 1000, "the tracks do nothing"
    if "filter" in name:
        assert err <= 1e-5 * float(np.abs(want).max()), err
    else:
        assert differ == 0, "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0)))


@functools.lru_cache(maxsize=None)
def plain_expected(oracle):
    onsets, _, gains = sv.layout(N)
    out = mix.score_chain_rows(list(oracle_rows(N, oracle)), onsets, sv.NT, None, gains)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def piece_expected(names, with_faders, oracle, buses=(), zero_column=None, master=None):
    """the two-instrument piece with the named tracks (None: a track without a circuit), once for the tests that share it"""
    onsets, _, gains = sv.layout(N)
    fxs = [None if name is None else tc.TRACKS[name] for name in names]
    want = tc.expected(oracle, list(oracle_rows(N, oracle)), onsets, sv.NT, fxs, tc.track_of(N, len(names)), 1, tc.faders(len(names)) if with_faders else None, gains=gains,
                       buses=[tc.TRACKS[b] for b in buses], track_sends=tc.levels(len(buses), len(names), zero_column) if buses else None,
                       master=None if master is None else tc.TRACKS[master])
    want.setflags(write=False)
    return want


def piece(names, with_faders=False, **kw):
    onsets, _, gains = sv.layout(N)
    d.configure(RATE)
    fxs = [None if name is None else tc.TRACKS[name] for name in names]
    return d.render_piece(voices(), onsets, durations(), DUR, None, gains, tracks=fxs, track_of=tc.track_of(N, len(names)),
                          faders=tc.faders(len(names)) if with_faders else None, **kw)


@pytest.mark.parametrize("engine", list(ENGINES))
def test_two_tracks_and_direct_voices_on_every_engine(engine, oracle):
    want = piece_expected(("clip", "echo"), False, oracle)
    of = tc.track_of(N, 2)
    assert (of == -1).sum() >= 2 and (of == 0).sum() >= 2 and (of == 1).sum() >= 2
    got = piece(("clip", "echo"), engine=ENGINES[engine])
    assert got.sampleRate == RATE and len(got) == 1
    held("clip+echo", got, want, plain_expected(oracle))


def test_three_tracks_with_one_echo_at_three_delays_are_one_program(oracle):
    d.configure(RATE)
    echoes = [mc.echo_of(300.25), mc.echo_of(411.5), mc.echo_of(257.75)]
    groups = render.track_programs(echoes, 1, RATE)
    assert len(groups) == 1 and groups[0][1] == [0, 1, 2] and groups[0][0].params.tolist() == [[300.25, 411.5, 257.75]], "ONE track program serves the three"
    onsets, _, gains = sv.layout(N)
    of, f = tc.track_of(N, 3), tc.faders(3)
    want = tc.expected(oracle, list(oracle_rows(N, oracle)), onsets, sv.NT, echoes, of, 1, f, gains=gains)
    held("three echoes", d.render_piece(voices(), onsets, durations(), DUR, None, gains, tracks=echoes, track_of=of, faders=f), want, plain_expected(oracle))
    # the same through programs of our own: one program of three instances, and the three tracks as programs of their own give the same bits
    ctx = runtime.Context(-1, RATE)
    uni = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(N)])
    rows = [np.asarray(r, dtype=np.float32) for r in oracle.render_instances(uni.words, sv.NV, uni.params, N, range(N))]
    one = groups[0][0]
    singles = [mc.unified_master(fx, 1) for fx in echoes]
    part, together, apart = ctx.build(uni.words), ctx.build(one.words), [ctx.build(s.words) for s in singles]
    try:
        run = lambda programs: ctx.render_score_parts([(part, sv.NV, N, uni.params)], [0] * N, onsets, sv.NT, None, gains,
                                                      tracks=dict(n_tracks=3, track_of=of, programs=programs, faders=f))
        got = run([(together, [0, 1, 2], one.params)])
        held("three echoes, one program", got, tc.expected(oracle, rows, onsets, sv.NT, echoes, of, 1, f, gains=gains))
        assert np.array_equal(bits(run([(p, [g], s.params) for g, (p, s) in enumerate(zip(apart, singles))])), bits(got))
        # the program's tracks in another order: its instances follow its list, the mix the tracks' numbers
        swapped = one.params[:, [2, 0, 1]].copy()
        assert np.array_equal(bits(run([(together, [2, 0, 1], swapped)])), bits(got))
    finally:
        for p in [part, together] + apart:
            p.close()
        ctx.close()


def test_a_track_without_a_circuit_with_a_fader_and_a_track_with_no_voices(oracle):
    """track 1 is a fader group; track 2, an echo, has no voices: its input is zeros and it adds its (zero) output all the same"""
    onsets, _, gains = sv.layout(N)
    of = tc.track_of(N, 2)
    fxs, f = [mc.clip, None, mc.echo], tc.faders(3)
    assert not (of == 2).any() and (of == 1).any()
    want = tc.expected(oracle, list(oracle_rows(N, oracle)), onsets, sv.NT, fxs, of, 1, f, gains=gains)
    d.configure(RATE)
    held("clip, fader group, silent echo", d.render_piece(voices(), onsets, durations(), DUR, None, gains, tracks=fxs, track_of=of, faders=f), want, plain_expected(oracle))
    # a fader group alone with a fader of 1 and everything in it is the plain piece
    alone = d.render_piece(voices(), onsets, durations(), DUR, None, gains, tracks=[None], track_of=[0] * N, faders=[1.0])
    assert np.array_equal(bits(np.stack(alone)), bits(plain_expected(oracle)))


def test_filter_tracks_as_one_program(oracle):
    names = ("lowpass", "lowpass", "clip")
    want = piece_expected(names, True, oracle)
    d.configure(RATE)
    assert [w for _, w in render.track_programs([tc.TRACKS[n] for n in names], 1, RATE)] == [[0, 1], [2]]
    held("filter x2 + clip", piece(names, True), want, plain_expected(oracle))


def placements():
    """name -> (voices, voice samples, onsets, gains, the call's keywords, the contract's keywords, the timeline's channels)"""
    onsets, _, gains = sv.layout(N)
    frac_onsets, fracs, frac_gains = frac_layout(N)
    mono = lambda: [sv.voice(k) for k in range(N)]
    rs = np.random.RandomState(5)
    places = rs.uniform(-3, 3, (N, 2))
    speakers = [[-1.5, 0], [1.5, 0], [0, 2]]
    pans = pans_for(N)
    return {
        "pans": (mono, onsets, gains, dict(pans=pans), dict(pans=pans), 2),
        "fracs_pans": (mono, frac_onsets, frac_gains, dict(pans=pans, fracs=fracs), dict(pans=pans, fracs=fracs), 2),
        "places": (mono, onsets, gains, dict(places=places, speakers=speakers), dict(taps=mix.space_taps(places, speakers, sample_rate=RATE)), 3),
        "stereo": (lambda: stc.voices_for(N, "in_turn"), onsets, gains, dict(pans=stc.stereo_pans(N, "in_turn"), stereo=True), dict(pans=stc.stereo_pans(N, "in_turn"), stereo=True), 2),
    }


@pytest.mark.parametrize("placement", ["pans", "fracs_pans", "places", "stereo"])
def test_tracks_behind_every_placement_with_a_circuit_a_channel(placement, oracle):
    """a track's timeline is the placement's chain over its voices; the echo track has a delay of its own per channel"""
    d.configure(RATE)
    make, onsets, gains, kw, contract_kw, channels = placements()[placement]
    rows = tc.oracle_voice_rows(oracle, make(), [sv.NV] * N)
    fxs, of, f = [CHANNEL_ECHOES[:channels], mc.clip, None], tc.track_of(N, 3), tc.faders(3)
    want = tc.expected(oracle, rows, onsets, sv.NT, fxs, of, channels, f, gains=gains, **contract_kw)
    before = tc.expected(oracle, rows, onsets, sv.NT, [None], [-1] * N, channels, gains=gains, **contract_kw)
    got = d.render_piece(make(), onsets, VOICE_DUR, DUR, None, gains, tracks=fxs, track_of=of, faders=f, **kw)
    assert len(got) == channels
    held("echo a channel + clip + group, " + placement, got, want, before)


def test_buses_fed_by_the_tracks_one_level_column_all_zero_and_a_master_behind(oracle):
    names, buses = ("clip", "echo", None), ("echo", "comb")
    want = piece_expected(names, True, oracle, buses, 1, "allpass")
    levels = tc.levels(2, 3, 1)
    assert not levels[1].any() and levels[0].all()
    got = piece(names, True, buses=[mc.echo, mc.comb], track_sends=levels, master=mc.allpass)
    held("tracks, buses and a master", got, want, plain_expected(oracle))
    # without the master; and the buses hear the tracks: it is not the piece without buses
    no_master = piece_expected(names, True, oracle, buses, 1)
    held("tracks and buses", piece(names, True, buses=[mc.echo, mc.comb], track_sends=levels), no_master)
    assert (bits(no_master) != bits(piece_expected(names, True, oracle))).sum() > 1000
    # buses behind a placement that per-note sends refuse
    onsets, fracs, gains = frac_layout(N)
    d.configure(RATE)
    mono = lambda: [sv.voice(k) for k in range(N)]
    rows = tc.oracle_voice_rows(oracle, mono(), [sv.NV] * N)
    of = tc.track_of(N, 2)
    want = tc.expected(oracle, rows, onsets, sv.NT, [mc.clip, None], of, 1, None, gains=gains, buses=[mc.echo], track_sends=tc.levels(1, 2), fracs=fracs)
    held("buses behind fracs", d.render_piece(mono(), onsets, VOICE_DUR, DUR, None, gains, fracs=fracs, tracks=[mc.clip, None], track_of=of, buses=[mc.echo], track_sends=tc.levels(1, 2)), want)


def test_tiles_repetition_and_a_call_without_tracks_afterwards(oracle):
    names = ("clip", "echo")
    want = piece_expected(names, True, oracle)
    call = lambda **kw: np.stack(piece(names, True, **kw))
    # 9000 bytes: two or three voices of 3092 and 4124 bytes a tile, at least five tiles: a track's chain spans several launches
    assert np.array_equal(bits(call(tile_bytes=9000)), bits(want)), "tiling changes the bits behind a track"
    assert np.array_equal(bits(call(tile_bytes=1)), bits(want)), "one voice a tile changes the bits behind a track"
    assert np.array_equal(bits(call()), bits(want)) and np.array_equal(bits(call()), bits(want)), "the second call differs"
    onsets, _, gains = sv.layout(N)
    d.configure(RATE)
    assert np.array_equal(bits(np.stack(d.render_piece(voices(), onsets, durations(), DUR, None, gains))), bits(plain_expected(oracle))), "a call without tracks is not what it was"
    # with lengths, on ONE context and ONE set of programs reused from call to call
    ctx = runtime.Context(-1, RATE)
    uni = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(N)])
    t = mc.unified_master(mc.echo, 1)
    part, track = ctx.build(uni.words), ctx.build(t.words)
    _, lengths, _ = sv.layout(N)
    of = tc.track_of(N, 2)
    try:
        run = lambda **kw: ctx.render_score_parts([(part, sv.NV, N, uni.params)], [0] * N, onsets, sv.NT, lengths, gains, **kw)
        with_tracks = dict(tracks=dict(n_tracks=2, track_of=of, programs=[(track, [1], t.params)]))
        before = run()
        first = run(**with_tracks)
        rows = [np.asarray(r, dtype=np.float32) for r in oracle.render_instances(uni.words, sv.NV, uni.params, N, range(N))]
        held("lengths", first, tc.expected(oracle, rows, onsets, sv.NT, [None, mc.echo], of, 1, None, lengths, gains))
        assert np.array_equal(bits(run(tile_bytes=7000, **with_tracks)), bits(first)) and np.array_equal(bits(run()), bits(before))
        assert (bits(first) != bits(before)).sum() > 1000
    finally:
        part.close()
        track.close()
        ctx.close()


def test_a_plan_budget_of_one_kilobyte_shared_over_the_destinations(oracle):
    """DUSP_SCORE_PLAN_KB=1: the call's budget goes to the tiles and, within a tile, to its destinations by their voices — every plan
    doubles its block until its lists fit its share, and the bits stay"""
    from conftest import knob_context
    ctx = knob_context(RATE, DUSP_SCORE_PLAN_KB=1)
    n = 37
    onsets, lengths, gains = sv.layout(n)
    d.configure(RATE)
    uni = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(n)])
    rows = [np.asarray(r, dtype=np.float32) for r in oracle.render_instances(uni.words, sv.NV, uni.params, n, range(n))]
    of = tc.track_of(n, 3)
    of = np.where(np.arange(n) % 9 == 0, of, 0).astype(np.int32)  # (most voices on track 0, a few on the other destinations)
    t = mc.unified_master(mc.clip, 1)
    part, track = ctx.build(uni.words), ctx.build(t.words)
    try:
        for tile_bytes in (0, 30000):
            got = ctx.render_score_parts([(part, sv.NV, n, uni.params)], [0] * n, onsets, sv.NT, lengths, gains, tile_bytes=tile_bytes,
                                         tracks=dict(n_tracks=3, track_of=of, programs=[(track, [0], t.params)], faders=tc.faders(3)))
            held("one kilobyte of plans, tile_bytes %d" % tile_bytes, got, tc.expected(oracle, rows, onsets, sv.NT, [mc.clip, None, None], of, 1, tc.faders(3), lengths, gains))
    finally:
        part.close()
        track.close()


def test_the_long_timeline_with_a_stateless_track(oracle):
    """10301 samples, 40 chunks and 61: the Clip track's render is cut into time segments and reads its input at segment offsets"""
    rs = np.random.RandomState(10301)
    onsets = rs.randint(1, mc.LONG - 10, N).astype(np.int64)
    onsets[N // 2] = 0
    gains = (0.05 + 1.9 * rs.random_sample(N)).astype(np.float32)
    of = tc.track_of(N, 2)
    want = tc.expected(oracle, list(oracle_rows(N, oracle)), onsets, mc.LONG, [mc.clip, mc.echo], of, 1, None, gains=gains)
    d.configure(RATE)
    got = d.render_piece(voices(), onsets, durations(), (mc.LONG + 0.5) / RATE, None, gains, tracks=[mc.clip, mc.echo], track_of=of)
    assert want[0, -2000:].any() and want[0, :2000].any()
    held("clip+echo, long", got, want)


def test_delivery_as_pcm_and_wav(oracle):
    """s16 / s24 frames and the peak of the piece with its tracks: the host's quantiser over the expected f32, for every normalise mode"""
    names = ("clip", "echo")
    want = piece_expected(names, True, oracle)
    onsets, _, gains = sv.layout(N)
    d.configure(RATE)
    with_tracks = dict(tracks=[tc.TRACKS[n] for n in names], track_of=tc.track_of(N, 2), faders=tc.faders(2))
    args = lambda: (voices(), onsets, durations(), DUR)
    peak_want = np.float32(np.abs(want).max())
    assert peak_want > 1.0  # (normalise = 1 has something to shrink)
    for depth in (16, 24):
        for normalise in (0, 1, 2):
            res = d.render_piece_pcm(*args(), depth, normalise, None, gains, **with_tracks)
            frames, frames_peak = wav.encode_frames(want, depth, normalise)
            assert res.data.dtype == frames.dtype and res.data.shape == frames.shape and res.bitDepth == depth and res.numberOfChannels == 1
            assert np.array_equal(res.data.view(np.uint8), frames.view(np.uint8)), (depth, normalise)
            assert np.float32(res.peak).view(np.uint32) == np.float32(frames_peak).view(np.uint32) == peak_want.view(np.uint32)
    file = d.render_piece_wav(*args(), 16, 0, None, gains, **with_tracks)
    assert file == wav.encode_wav([c for c in want], RATE, 16) and file[:4] == b"RIFF"


def test_render_score_with_tracks_is_render_piece_of_one_structure(oracle):
    d.configure(RATE)
    onsets, lengths, gains = sv.layout(N)
    mono = lambda: [sv.voice(k) for k in range(N)]
    of = tc.track_of(N, 2)
    with_tracks = dict(tracks=[mc.echo, mc.comb], track_of=of, faders=tc.faders(2))
    want = np.stack(d.render_piece(mono(), onsets, VOICE_DUR, DUR, lengths, gains, **with_tracks))
    got = d.render_score(mono(), onsets, VOICE_DUR, DUR, lengths, gains, **with_tracks)
    assert got.sampleRate == RATE and len(got) == 1 and np.array_equal(bits(np.stack(got)), bits(want))
    rows = tc.oracle_voice_rows(oracle, mono(), [sv.NV] * N)
    held("echo+comb over a score", want, tc.expected(oracle, rows, onsets, sv.NT, [mc.echo, mc.comb], of, 1, tc.faders(2), lengths, gains))
    assert len(d.render_score(mono(), onsets, VOICE_DUR, 0, **with_tracks)) == 0
    pcm = d.render_score_pcm(mono(), onsets, VOICE_DUR, DUR, 16, 1, lengths, gains, **with_tracks)
    assert np.array_equal(pcm.data, wav.encode_frames(want, 16, 1)[0])


# ---- the device entry alone -------------------------------------------------------------------------------------------------------------

SENTINEL, GUARD = -12345.678, 64


def planted(n, seed):
    rs = np.random.RandomState(seed)
    a = (rs.standard_normal(n) * 10.0 ** rs.randint(-3, 4, n)).astype(np.float32)
    for j, v in enumerate([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -5e-39, np.finfo(np.float32).max]):
        a[(7 * j + 3 + seed) % n] = v
    return a


@pytest.mark.parametrize("n", [1, 3, 4, 1027])
def test_the_mix_entry_alone(n):
    """T = 1 and 8, B = 0 .. 4, with and without faders, raw and not, out of place into buffers off a 16-byte boundary (one float a lane)
    and in place on boundaries (four floats a lane and a tail; with B > 1 and n % 4 != 0 the feeds behind the first are off them)"""
    import torch
    ctx = runtime.Context(-1, RATE)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for T in (1, 8):
            for B in range(5):
                for variant in range(4):
                    with_faders, raw, aligned = variant & 1, variant >> 1, (variant + B) & 1
                    direct, ys = planted(n, 1 + B), [planted(n, 10 + g + T) for g in range(T)]
                    faders = np.array([0.0, -0.0, 1.0, -0.75, 1e-30, 3e20, 0.6, 2.0][:T], dtype=np.float32) if with_faders else None
                    levels = np.array([[0.0, -0.0, 1.0, -0.5, 1e-30, 3e20, 0.25, 1.5][(b + g) % 8] for b in range(B) for g in range(T)], dtype=np.float32).reshape(B, T) if B else None
                    feed0 = planted(max(B, 1) * n, 40 + B).reshape(max(B, 1), n)[:B]
                    want, want_feeds = mix.track_mix(direct[None], [y[None] for y in ys], faders, levels)
                    skip = 0 if aligned else 1
                    d_ys = [torch.from_numpy(np.concatenate([np.zeros(skip, np.float32), y])).cuda() for y in ys]
                    if aligned:  # in place: out is direct, feed_out is feed_init (the feeds then start from feed0)
                        d_direct = torch.from_numpy(direct.copy()).cuda()
                        d_feed = torch.from_numpy(feed0.reshape(-1).copy() if B else np.zeros(1, np.float32)).cuda()
                        assert d_direct.data_ptr() % 16 == 0 and d_feed.data_ptr() % 16 == 0 and all(t.data_ptr() % 16 == 0 for t in d_ys)
                        ctx.score_tracks_mix(d_direct.data_ptr(), [t.data_ptr() for t in d_ys], n, d_direct.data_ptr(), faders, levels, d_feed.data_ptr() if B else None,
                                             d_feed.data_ptr() if B else None, raw=raw, stream=stream)
                        torch.cuda.synchronize()
                        got, got_feeds = d_direct.cpu().numpy(), d_feed.cpu().numpy()[:B * n].reshape(B, n)
                        want_feeds = np.stack([loop_feed(feed0[b], ys, faders, levels[b]) for b in range(B)]) if B else want_feeds
                    else:
                        d_direct = torch.from_numpy(np.concatenate([np.zeros(3, np.float32), direct])).cuda()
                        d_out = torch.full((GUARD + 1 + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
                        d_feed = torch.full((GUARD + 3 + max(B, 1) * n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
                        ctx.score_tracks_mix(d_direct.data_ptr() + 12, [t.data_ptr() + 4 for t in d_ys], n, d_out.data_ptr() + 4 * (GUARD + 1), faders, levels,
                                             d_feed.data_ptr() + 4 * (GUARD + 3) if B else None, None, raw=raw, stream=stream)
                        torch.cuda.synchronize()
                        out, feed = d_out.cpu().numpy(), d_feed.cpu().numpy()
                        assert (out[:GUARD + 1] == np.float32(SENTINEL)).all() and (out[GUARD + 1 + n:] == np.float32(SENTINEL)).all(), "floats beside the output were written"
                        assert (feed[:GUARD + 3] == np.float32(SENTINEL)).all() and (feed[GUARD + 3 + B * n:] == np.float32(SENTINEL)).all(), "floats beside the feeds were written"
                        got, got_feeds = out[GUARD + 1:GUARD + 1 + n], feed[GUARD + 3:GUARD + 3 + B * n].reshape(B, n)
                    want_out = want[0] if raw else mix.bus_return(want, [])[0]
                    where = (n, T, B, variant)
                    assert same(got, want_out), where  # (bit patterns, so -0 and +0 too; for NaN, the positions)
                    assert same(got_feeds, want_feeds.reshape(B, n)), where
        assert ctx.score_last_ms()[0] > 0
    finally:
        ctx.close()


def loop_feed(start, ys, faders, levels):
    """a feed that starts from `start`: the contract's chain, array by array"""
    acc = start.copy()
    with np.errstate(all="ignore"):
        for g, y in enumerate(ys):
            term = y if faders is None else y * faders[g]
            acc = acc + term * levels[g]
    return acc


# ---- the C entry, through ctypes -------------------------------------------------------------------------------------------------------

def test_the_c_entry_refuses_before_anything_renders():
    d.configure(RATE)
    L = runtime.load()
    ctx, other = runtime.Context(-1, RATE), runtime.Context(-1, RATE)
    two = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(2)])
    build = lambda c, outlet, engine=runtime.ENGINE_AUTO: c.build(descriptor.extract(outlet).words, engine)
    echo = mc.unified_master([mc.echo_of(300.25)], 1)
    with_param = mc.unified_master([mc.echo_of(300.25), mc.echo_of(411.5)], 2)  # (a program with one parameter: the delay)
    programs = dict(part=ctx.build(two.words), good=ctx.build(echo.words), good2=ctx.build(echo.words), good3=ctx.build(echo.words), no_input=build(ctx, sv.voice(5)),
                    two_inputs=build(ctx, d.Sum(d.MasterInput(), d.HostSource(np.zeros(4)))), wide=build(ctx, d.Pan(d.MasterInput(), 0.25)),
                    resumable=ctx.build(echo.words, runtime.ENGINE_AUTO | runtime.ENGINE_RESUMABLE), elsewhere=other.build(echo.words), param=ctx.build(with_param.words))
    parts = (runtime.ScorePart * 1)(runtime.ScorePart(programs["part"]._h, 2, sv.NV, two.params.ctypes.data))
    part_of, onsets = np.zeros(2, dtype=np.uint32), np.array([0, 40], dtype=np.int64)
    out = np.full((1, 1024), 7, dtype=np.float32)
    ones = np.ones((4, 8), dtype=np.float32)
    who = "dusp_render_host_score_piece_tracks: "
    keep = []

    def call(circuits, track_of=(0, -1), n_tracks=1, faders=None, track_sends=None, buses=None, sends=None, master=None, n_total=1024, n_programs=None, null_of=False):
        table = (runtime.ScoreTrackProgram * max(len(circuits), 1))()
        for p, (prog, which) in enumerate(circuits):
            which = np.array(which, dtype=np.uint32)
            keep.append(which)
            table[p] = runtime.ScoreTrackProgram(prog._h if prog is not None else None, len(which), which.ctypes.data if len(which) else None, None)
        of = np.array(track_of, dtype=np.int32)
        routed = runtime.ScoreTracks(n_tracks, None if null_of else of.ctypes.data, len(circuits) if n_programs is None else n_programs, ctypes.addressof(table),
                                     None if faders is None else faders.ctypes.data, None if track_sends is None else track_sends.ctypes.data)
        into = None
        if buses is not None:
            bus_table = (runtime.ScoreMaster * max(len(buses), 1))(*[runtime.ScoreMaster(b._h, None) for b in buses])
            into = runtime.ScoreBuses(len(buses), ctypes.addressof(bus_table), None if sends is None else sends.ctypes.data)
        through = runtime.ScoreMaster(master._h, None) if master is not None else None
        return L.dusp_render_host_score_piece_tracks(parts, 1, 2, part_of.ctypes.data, onsets.ctypes.data, None, None, None, ctypes.addressof(routed),
                                                     ctypes.addressof(into) if into is not None else None, ctypes.addressof(through) if through is not None else None, n_total, 0, 0, 0,
                                                     out.ctypes.data, None)

    P = programs
    nan_fader, nan_level = np.array([1, np.nan], dtype=np.float32), ones[:2, :2].copy()
    nan_level[1, 0] = np.inf
    try:
        for kw, needle, status in [
            (dict(circuits=[], n_tracks=0), "a call has 1 .. 8 tracks, not 0", -1),
            (dict(circuits=[], n_tracks=9), "a call has 1 .. 8 tracks, not 9", -1),
            (dict(circuits=[], null_of=True), "the tracks' h_track_of is NULL", -1),
            (dict(circuits=[], track_of=(0, 1)), "voice 1 names track 1 of 1: track_of holds -1 (straight to the mix) or a track, 0 .. 0", -1),
            (dict(circuits=[], track_of=(-2, 0)), "voice 0 names track -2 of 1", -1),
            (dict(circuits=[], n_tracks=2, faders=nan_fader), "the fader of track 1 is not finite", -1),
            (dict(circuits=[], track_sends=ones), "track_sends without buses", -1),
            (dict(circuits=[], buses=[P["good"]]), "buses without track_sends", -1),
            (dict(circuits=[], buses=[P["good"]], sends=ones, track_sends=ones), "sends and tracks do not go together", -2),
            (dict(circuits=[], n_tracks=2, buses=[P["good"], P["good2"]], track_sends=nan_level), "the level of track 0 into bus 1 is not finite", -1),
            (dict(circuits=[], buses=[], track_sends=ones), "a call has 1 .. 4 buses, not 0", -1),
            (dict(circuits=[(P["good"], [0]), (P["no_input"], [1])], n_tracks=2), "a track program reads exactly one input stream (the track timeline's channel), this program has 0", -1),
            (dict(circuits=[(P["two_inputs"], [0])]), "a track program reads exactly one input stream (the track timeline's channel), this program has 2", -1),
            (dict(circuits=[(P["wide"], [0])]), "a track program has one output channel, this program has 2", -1),
            (dict(circuits=[(P["good"], [0]), (P["resumable"], [1])], n_tracks=2), "a resumable program (DUSP_ENGINE_RESUMABLE) is not a track program", -2),
            (dict(circuits=[(P["elsewhere"], [0])]), "track program 0 was built on another context", -1),
            (dict(circuits=[(P["good"], [0]), (P["part"], [1])], n_tracks=2), "track program 1 is also part 0", -1),
            (dict(circuits=[(P["param"], [0])]), "track program 0 has parameters but its h_params is NULL", -1),
            (dict(circuits=[(None, [0])]), "track program 0's program is NULL", -1),
            (dict(circuits=[(P["good"], [0])], n_total=(1 << 31) + 1), "track program 0 renders channels x timeline samples, which must not exceed 2^31", -1),
            (dict(circuits=[(P["good"], [0, 1, 2])], n_tracks=3, n_total=1 << 30), "track program 0 renders (tracks x channels) x timeline samples, which must not exceed 2^31", -1),
            (dict(circuits=[(P["good"], [0])], master=P["good"]), "track program 0 is also the master", -1),
            (dict(circuits=[(P["good"], [0])], buses=[P["good2"], P["good"]], track_sends=ones), "track program 0 is also bus 1", -1),
            (dict(circuits=[(P["good"], [0]), (P["good2"], [1]), (P["good"], [2])], n_tracks=3), "track programs 0 and 2 are the same program", -1),
            (dict(circuits=[(P["good"], [])]), "track program 0 lists no tracks", -1),
            (dict(circuits=[(P["good"], [1])]), "track program 0 lists track 1 of 1", -1),
            (dict(circuits=[(P["good"], [0]), (P["good2"], [1, 0])], n_tracks=2), "track program 1 lists track 0, which has a circuit already", -1),
            (dict(circuits=[(P["good"], [0]), (P["good2"], [0])], n_programs=2), "2 track programs for 1 tracks", -1),
        ]:
            assert call(**kw) == status, needle
            message = L.dusp_last_error(ctx._h).decode()
            assert message.startswith(who) and needle in message, message
            assert (out == 7).all(), "a refused call wrote to h_out"
        # the strings the hosts share with the library
        for kw, text in ((dict(circuits=[], n_tracks=9), mix.TRACKS_COUNT % 9), (dict(circuits=[], track_of=(0, 3)), mix.TRACKS_TRACK_OF_RANGE % (1, 3, 1, 0)),
                         (dict(circuits=[], n_tracks=2, faders=nan_fader), mix.TRACKS_FADER_NOT_FINITE % 1), (dict(circuits=[], track_sends=ones), mix.TRACKS_SENDS_WITHOUT_BUSES),
                         (dict(circuits=[], buses=[P["good"]]), mix.TRACKS_BUSES_WITHOUT_SENDS), (dict(circuits=[], buses=[P["good"]], sends=ones, track_sends=ones), mix.TRACKS_WITH_SENDS),
                         (dict(circuits=[], n_tracks=2, buses=[P["good"], P["good2"]], track_sends=nan_level), mix.TRACKS_LEVEL_NOT_FINITE % (0, 1))):
            assert call(**kw) < 0 and L.dusp_last_error(ctx._h).decode() == text.replace("dusp-hip: ", who)
        # what is a track renders; without tracks the entry is dusp_render_host_score_piece_buses
        assert call(circuits=[(P["good"], [0])]) == 0, L.dusp_last_error(ctx._h).decode()
        with_track = out.copy()
        assert L.dusp_render_host_score_piece_tracks(parts, 1, 2, part_of.ctypes.data, onsets.ctypes.data, None, None, None, None, None, None, 1024, 0, 0, 0, out.ctypes.data, None) == 0
        assert np.array_equal(bits(out), bits(ctx.render_score_parts([(P["part"], sv.NV, 2, two.params)], [0, 0], onsets, 1024)))
        assert (bits(with_track) != bits(out)).sum() > 100 and not (with_track == 7).any()
        # the device entry's own
        import torch
        buf = torch.zeros(64, dtype=torch.float32, device="cuda")
        p = buf.data_ptr()
        ptrs = (ctypes.c_void_p * 8)(*([p] * 8))
        none = (ctypes.c_void_p * 8)()
        one, bad = np.ones((4, 8), dtype=np.float32), np.full((4, 8), np.nan, dtype=np.float32)
        entry = lambda *args: L.dusp_score_tracks_mix_device(ctx._h, *args, None)
        for args, needle in [((p, ptrs, 0, None, 0, None, 8, 0, p, None, None), "a call has 1 .. 8 tracks, not 0"), ((p, ptrs, 9, None, 0, None, 8, 0, p, None, None), "a call has 1 .. 8 tracks, not 9"),
                             ((p, ptrs, 1, None, 5, one.ctypes.data, 8, 0, p, None, p), "a call has 0 .. 4 buses, not 5"), ((None, ptrs, 1, None, 0, None, 8, 0, p, None, None), "NULL buffer"),
                             ((p, none, 1, None, 0, None, 8, 0, p, None, None), "NULL buffer"), ((p, ptrs, 1, None, 1, one.ctypes.data, 8, 0, p, None, None), "NULL buffer"),
                             ((p, ptrs, 1, None, 1, None, 8, 0, p, None, p), "NULL buffer"), ((p, ptrs, 1, None, 0, None, 0, 0, p, None, None), "need 1..2^31 floats"),
                             ((p, ptrs, 1, None, 0, None, 8, 0, p + 2, None, None), "4-byte aligned"), ((p, ptrs, 2, bad.ctypes.data, 0, None, 8, 0, p, None, None), "the fader of track 0 is not finite"),
                             ((p, ptrs, 2, None, 1, bad.ctypes.data, 8, 0, p, None, p), "the level of track 0 into bus 0 is not finite")]:
            assert entry(*args) == -1 and needle in L.dusp_last_error(ctx._h).decode(), needle
        torch.cuda.synchronize()
        assert not buf.cpu().numpy().any()  # (nothing ran)
    finally:  # (programs before their contexts, whatever failed)
        for prog in programs.values():
            prog.close()
        ctx.close()
        other.close()
