"""Effect sends on the device (dusp_render_host_score_piece_buses, dusp_score_rows_send_device, dusp_score_return_device; DESIGN.md
6.15).  The expected value is the contract over the CPU oracle's renders: the voices' rows from the oracle, as the piece tests take
them (test_piece_host.oracle_rows) -> mix.score_chain_sends -> every bus rendered over its send timeline by the oracle
(master_cases.oracle_master) -> mix.bus_return (-> the oracle's master).  Bit for bit; a Filter bus would be held within 1e-5 of the
expected signal's largest magnitude, the project's figure for Filter graphs.  tests/test_sends_host.py anchors the contract."""
import ctypes
import functools

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
import send_cases as sc
from pan_cases import pans_for
from dusp_amd import descriptor, mix, runtime, wav
from test_piece_host import NV_SAW, bits, interleaved_voice, oracle_rows

pytestmark = pytest.mark.gpu

RATE = sv.SAMPLE_RATE
ENGINES = {"auto": runtime.ENGINE_AUTO, "chunk": runtime.ENGINE_CHUNK, "wave": runtime.ENGINE_WAVE}
N = 13
DUR, VOICE_DUR = (sv.NT + 0.5) / RATE, (sv.NV + 0.5) / RATE
CHANNEL_ECHOES = [mc.echo_of(300.25), mc.echo_of(411.5)]  # a bus a channel: one program, the delay its parameter


def voices(n=N):
    return [interleaved_voice(k) for k in range(n)]


def durations(n=N):
    return [((sv.NV if k % 2 == 0 else NV_SAW) + 0.5) / RATE for k in range(n)]


def held(name, got, want, before):
    """bit for bit (a Filter bus: within 1e-5 of the expected signal's largest magnitude), and the buses are heard"""
    got = np.stack(got) if not isinstance(got, np.ndarray) else got
    assert got.dtype == np.float32 and got.shape == want.shape
    differ = int((bits(got) != bits(want)).sum())
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: %d samples differ in bits, max |err| %.3g, max |want| %.3g" % (name, differ, err, float(np.abs(want).max())))
    assert (bits(want) != bits(before)).any(axis=0).sum() > 1000, "the buses do nothing"
    if "filter" in name:
        assert err <= 1e-5 * float(np.abs(want).max()), err
    else:
        assert differ == 0, "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0)))


@functools.lru_cache(maxsize=None)
def piece_expected(names, zero_column, master, oracle):
    """the two-instrument piece with the named buses -> (expected, the dry piece as delivered), once for the tests that share it"""
    onsets, _, gains = sv.layout(N)
    fxs = [sc.BUSES[name] for name in names]
    want, dry = sc.expected(oracle, list(oracle_rows(N, oracle)), onsets, sv.NT, fxs, sc.levels(N, len(names), zero_column), None, gains, master=master)
    want.setflags(write=False)
    dry.setflags(write=False)
    return want, dry


@pytest.mark.parametrize("engine", list(ENGINES))
def test_an_echo_bus_on_every_engine(engine, oracle):
    want, dry = piece_expected(("echo",), None, None, oracle)
    onsets, _, gains = sv.layout(N)
    d.configure(RATE)
    got = d.render_piece(voices(), onsets, durations(), DUR, None, gains, engine=ENGINES[engine], buses=[mc.echo], sends=sc.levels(N))
    assert got.sampleRate == RATE and len(got) == 1
    held("echo", got, want, dry)


def test_three_buses_with_levels_of_their_own_one_column_all_zero(oracle):
    want, dry = piece_expected(("echo", "comb", "clip"), 1, None, oracle)
    onsets, _, gains = sv.layout(N)
    levels = sc.levels(N, 3, 1)
    assert not levels[1].any() and levels[0].any() and levels[2].any() and (levels[0] != levels[2]).any()
    d.configure(RATE)
    held("echo+comb+clip", d.render_piece(voices(), onsets, durations(), DUR, None, gains, buses=[mc.echo, mc.comb, mc.clip], sends=levels), want, dry)
    # the bus that is sent nothing is rendered all the same and returns zeros: the mix is the one without it
    two = d.render_piece(voices(), onsets, durations(), DUR, None, gains, buses=[mc.echo, mc.clip], sends=levels[[0, 2]])
    assert np.array_equal(bits(np.stack(two)), bits(want))
    # four buses, the most a call takes
    four, _ = sc.expected(oracle, list(oracle_rows(N, oracle)), onsets, sv.NT, [mc.echo, mc.comb, mc.clip, mc.allpass], sc.levels(N, 4), None, gains)
    held("four", d.render_piece(voices(), onsets, durations(), DUR, None, gains, buses=[mc.echo, mc.comb, mc.clip, mc.allpass], sends=sc.levels(N, 4)), four, dry)


@pytest.mark.parametrize("placement", ["rows", "pans"])
def test_a_bus_a_channel_behind_two_channel_rows_and_behind_pans(placement, oracle):
    """the echo with a delay of its own per channel: channel c's bus hears channel c's sends alone; behind pans the send is post-pan"""
    d.configure(RATE)
    if placement == "rows":
        n, make, kw = 5, lambda: [mc.stereo_voice(k) for k in range(5)], {}
    else:
        n, make, kw = N, lambda: [sv.voice(k) for k in range(N)], dict(pans=pans_for(N))
    onsets, _, gains = sv.layout(n)
    uni = descriptor.unify([descriptor.extract(v) for v in make()])
    rows = [np.asarray(r, dtype=np.float32) for r in oracle.render_instances(uni.words, sv.NV, uni.params, n, range(n))]
    levels = sc.levels(n, 2)
    want, dry = sc.expected(oracle, rows, onsets, sv.NT, [CHANNEL_ECHOES, mc.clip], levels, None, gains, pans=kw.get("pans"))
    assert want.shape == (2, sv.NT)
    got = d.render_piece(make(), onsets, VOICE_DUR, DUR, None, gains, buses=[CHANNEL_ECHOES, mc.clip], sends=levels, **kw)
    held("echo a channel + clip, " + placement, got, want, dry)
    d.configure(RATE)
    assert np.array_equal(bits(np.stack(d.render_piece(make(), onsets, VOICE_DUR, DUR, None, gains, **kw))), bits(dry)), "the dry piece is not the oracle's"


def test_buses_and_a_master(oracle):
    want, dry = piece_expected(("echo", "clip"), None, mc.allpass, oracle)
    onsets, _, gains = sv.layout(N)
    d.configure(RATE)
    got = d.render_piece(voices(), onsets, durations(), DUR, None, gains, buses=[mc.echo, mc.clip], sends=sc.levels(N, 2), master=mc.allpass)
    held("echo+clip under an allpass master", got, want, dry)
    # the master hears the buses: it is not the master over the dry mix
    assert (bits(want) != bits(mc.oracle_master(oracle, mc.allpass, dry))).sum() > 1000


def test_tiles_repetition_and_a_call_without_buses_afterwards(oracle):
    want, dry = piece_expected(("echo",), None, None, oracle)
    d.configure(RATE)
    onsets, _, gains = sv.layout(N)
    call = lambda **kw: np.stack(d.render_piece(voices(), onsets, durations(), DUR, None, gains, **kw))
    with_bus = dict(buses=[mc.echo], sends=sc.levels(N))
    # 9000 bytes: two or three voices of 3092 and 4124 bytes a tile, at least five tiles: a voice's chains span several send launches
    assert np.array_equal(bits(call(tile_bytes=9000, **with_bus)), bits(want)), "tiling changes the bits behind a bus"
    assert np.array_equal(bits(call(tile_bytes=1, **with_bus)), bits(want)), "one voice a tile changes the bits behind a bus"
    assert np.array_equal(bits(call(**with_bus)), bits(want)) and np.array_equal(bits(call(**with_bus)), bits(want)), "the second call differs"
    assert np.array_equal(bits(call()), bits(dry)), "a call without buses is not what it was before one with"
    # the same on ONE context and ONE set of programs, reused from call to call
    ctx = runtime.Context(-1, RATE)
    uni = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(N)])
    b = mc.unified_master(mc.echo, 1)
    part, bus = ctx.build(uni.words), ctx.build(b.words)
    try:
        run = lambda **kw: ctx.render_score_parts([(part, sv.NV, N, uni.params)], [0] * N, onsets, sv.NT, None, gains, **kw)
        before = run()
        first = run(buses=[(bus, b.params)], sends=sc.levels(N))
        assert np.array_equal(bits(run(buses=[(bus, b.params)], sends=sc.levels(N), tile_bytes=7000)), bits(first)) and np.array_equal(bits(run()), bits(before))
        assert (bits(first) != bits(before)).sum() > 1000
        with pytest.raises(runtime.DuspHipError, match="last render was a mix"):
            bus.state(0)
    finally:
        part.close()
        bus.close()
        ctx.close()


def test_delivery_as_pcm_and_wav(oracle):
    """s16 / s24 frames and the peak of the piece with its bus: the host's quantiser over the expected f32, for every normalise mode"""
    want, _ = piece_expected(("echo",), None, None, oracle)
    d.configure(RATE)
    onsets, _, gains = sv.layout(N)
    args = lambda: (voices(), onsets, durations(), DUR)
    with_bus = dict(buses=[mc.echo], sends=sc.levels(N))
    peak_want = np.float32(np.abs(want).max())
    assert peak_want > 1.0  # (normalise = 1 has something to shrink)
    for depth in (16, 24):
        for normalise in (0, 1, 2):
            res = d.render_piece_pcm(*args(), depth, normalise, None, gains, **with_bus)
            frames, frames_peak = wav.encode_frames(want, depth, normalise)
            assert res.data.dtype == frames.dtype and res.data.shape == frames.shape and res.bitDepth == depth and res.numberOfChannels == 1
            assert np.array_equal(res.data.view(np.uint8), frames.view(np.uint8)), (depth, normalise)
            assert np.float32(res.peak).view(np.uint32) == np.float32(frames_peak).view(np.uint32) == peak_want.view(np.uint32)
    file = d.render_piece_wav(*args(), 16, 0, None, gains, **with_bus)
    assert file == wav.encode_wav([c for c in want], RATE, 16) and file[:4] == b"RIFF"


def test_render_score_with_buses_is_render_piece_of_one_structure(oracle):
    d.configure(RATE)
    onsets, lengths, gains = sv.layout(N)
    mono = lambda: [sv.voice(k) for k in range(N)]
    with_bus = dict(buses=[mc.echo, mc.comb], sends=sc.levels(N, 2))
    want = np.stack(d.render_piece(mono(), onsets, VOICE_DUR, DUR, lengths, gains, **with_bus))
    got = d.render_score(mono(), onsets, VOICE_DUR, DUR, lengths, gains, **with_bus)
    assert got.sampleRate == RATE and len(got) == 1 and np.array_equal(bits(np.stack(got)), bits(want))
    uni = descriptor.unify([descriptor.extract(v) for v in mono()])
    rows = [np.asarray(r, dtype=np.float32) for r in oracle.render_instances(uni.words, sv.NV, uni.params, N, range(N))]
    expected, dry = sc.expected(oracle, rows, onsets, sv.NT, [mc.echo, mc.comb], sc.levels(N, 2), lengths, gains)
    held("echo+comb over a score", want, expected, dry)
    # ... and the score without buses, which goes the contiguous way, is the dry mix
    assert np.array_equal(bits(np.stack(d.render_score(mono(), onsets, VOICE_DUR, DUR, lengths, gains))), bits(dry))
    assert len(d.render_score(mono(), onsets, VOICE_DUR, 0, **with_bus)) == 0
    pcm = d.render_score_pcm(mono(), onsets, VOICE_DUR, DUR, 16, 1, lengths, gains, **with_bus)
    assert np.array_equal(pcm.data, wav.encode_frames(want, 16, 1)[0])


# ---- the device entries alone -----------------------------------------------------------------------------------------------------------

SENTINEL, GUARD = -12345.678, 64


@pytest.mark.parametrize("panned", [False, True], ids=["rows", "pan"])
@pytest.mark.parametrize("n_buses", [1, 2, 3, 4])
def test_the_send_and_return_entries_alone(n_buses, panned):
    """planted rows (NaN, Inf, -0, subnormals) of 1, 255, 257 and 773 samples; the chain in two launches, the second in place over a
    window that starts in the middle of a group (its first voice begins at sample 300); then the return over the send timelines"""
    import torch
    from test_piece_host import planted_rows, same
    rows, onsets, lengths, gains, n_total = planted_rows(n_ch=1 if panned else 2)
    n, n_ch = len(rows), 2
    onsets = np.array(onsets)
    cut = 5
    onsets[cut:] = np.maximum(onsets[cut:], 300)  # the second launch's voices: none before sample 300
    rs = np.random.RandomState(40 + n_buses)
    levels = (rs.random_sample((n_buses, n)) * 2 - 0.5).astype(np.float32)
    levels[:, 2] = 0
    pans = np.linspace(-1, 1, n).astype(np.float32) if panned else None
    want_dry, want_send = mix.score_chain_sends(rows, onsets, n_total, levels, lengths, gains, pans)
    ctx = runtime.Context(-1, RATE)
    try:
        tensors = [torch.from_numpy(np.array(r).reshape(-1)).cuda() for r in rows]
        pointers, samples = [t.data_ptr() for t in tensors], [r.shape[1] for r in rows]
        d_gains = torch.from_numpy(np.array(gains)).cuda()
        row, srow = n_ch * n_total, n_buses * n_ch * n_total
        d_out = torch.full((GUARD + 1 + row + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")  # (one float past a 16-byte boundary)
        d_snd = torch.full((GUARD + 3 + srow + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        p_out, p_snd = d_out.data_ptr() + 4 * (GUARD + 1), d_snd.data_ptr() + 4 * (GUARD + 3)
        stream = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()
        kw = dict(pans=None if pans is None else pans[:cut])
        ctx.score_rows_send(pointers[:cut], samples[:cut], 1 if panned else n_ch, onsets[:cut], levels[:, :cut], n_total, p_out, p_snd, lengths[:cut],
                            d_gains.data_ptr(), raw=True, stream=stream, **kw)
        kw = dict(pans=None if pans is None else pans[cut:])
        ctx.score_rows_send(pointers[cut:], samples[cut:], 1 if panned else n_ch, onsets[cut:], levels[:, cut:], n_total, p_out, p_snd, lengths[cut:],
                            d_gains.data_ptr() + 4 * cut, p_out, p_snd, raw=True, stream=stream, **kw)
        kernel_ms, plan_ms, upload_ms = ctx.score_last_ms()
        assert kernel_ms > 0 and plan_ms >= 0
        torch.cuda.synchronize()
        out, snd = d_out.cpu().numpy(), d_snd.cpu().numpy()
        for a, lo, size in ((out, GUARD + 1, row), (snd, GUARD + 3, srow)):
            assert (a[:lo] == np.float32(SENTINEL)).all() and (a[lo + size:] == np.float32(SENTINEL)).all(), "floats beside an output were written"
        got_dry, got_send = out[GUARD + 1:GUARD + 1 + row].reshape(n_ch, n_total), snd[GUARD + 3:GUARD + 3 + srow].reshape(n_buses, n_ch, n_total)
        assert same(got_dry, want_dry) and same(got_send, want_send)
        assert np.isnan(want_send).any() and np.isinf(want_send).any()
        # the return: the send timelines as the buses' outputs, out of place into an unaligned buffer (one float a lane) ...
        d_mix = torch.full((GUARD + 2 + row + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        wets = [p_snd + 4 * b * row for b in range(n_buses)]
        ctx.score_return(p_out, wets, row, d_mix.data_ptr() + 4 * (GUARD + 2), raw=False, stream=stream)
        assert ctx.score_last_ms()[0] > 0
        torch.cuda.synchronize()
        mixed = d_mix.cpu().numpy()
        assert (mixed[:GUARD + 2] == np.float32(SENTINEL)).all() and (mixed[GUARD + 2 + row:] == np.float32(SENTINEL)).all()
        want_mix = mix.bus_return(want_dry, list(want_send))
        assert same(mixed[GUARD + 2:GUARD + 2 + row].reshape(n_ch, n_total), want_mix) and not np.isnan(want_mix).any()
        # ... and raw, in place, on 16-byte boundaries (four floats a lane and a tail: 2 x 1301 floats)
        a_dry = torch.from_numpy(want_dry.reshape(-1).copy()).cuda()
        a_wets = [torch.from_numpy(np.ascontiguousarray(want_send[b]).reshape(-1)).cuda() for b in range(n_buses)]
        assert all(t.data_ptr() % 16 == 0 for t in [a_dry] + a_wets) and row % 4 != 0
        ctx.score_return(a_dry.data_ptr(), [t.data_ptr() for t in a_wets], row, a_dry.data_ptr(), raw=True, stream=stream)
        torch.cuda.synchronize()
        raw_mix = mix.bus_return(want_dry, list(want_send), raw=True)
        got_raw = a_dry.cpu().numpy().reshape(n_ch, n_total)
        assert same(got_raw, raw_mix) and np.array_equal(np.signbit(got_raw), np.signbit(raw_mix))
    finally:
        ctx.close()


# ---- the C entry, through ctypes -------------------------------------------------------------------------------------------------------

def test_the_c_entry_refuses_before_anything_renders():
    d.configure(RATE)
    L = runtime.load()
    ctx, other = runtime.Context(-1, RATE), runtime.Context(-1, RATE)
    two = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(2)])
    build = lambda c, outlet, engine=runtime.ENGINE_AUTO: c.build(descriptor.extract(outlet).words, engine)
    echo = mc.unified_master(CHANNEL_ECHOES[:1], 1)
    with_param = mc.unified_master(CHANNEL_ECHOES[:2], 2)  # (a program with one parameter: the delay)
    programs = dict(part=ctx.build(two.words), good=ctx.build(echo.words), good2=ctx.build(echo.words), no_input=build(ctx, sv.voice(5)),
                    two_inputs=build(ctx, d.Sum(d.MasterInput(), d.HostSource(np.zeros(4)))), wide=build(ctx, d.Pan(d.MasterInput(), 0.25)),
                    resumable=ctx.build(echo.words, runtime.ENGINE_AUTO | runtime.ENGINE_RESUMABLE), elsewhere=other.build(echo.words), param=ctx.build(with_param.words))
    parts = (runtime.ScorePart * 1)(runtime.ScorePart(programs["part"]._h, 2, sv.NV, two.params.ctypes.data))
    part_of, onsets = np.zeros(2, dtype=np.uint32), np.array([0, 40], dtype=np.int64)
    out = np.full((1, 1024), 7, dtype=np.float32)
    ones = np.ones((4, 2), dtype=np.float32)
    fracs, pans = np.zeros(2), np.zeros(2, dtype=np.float32)
    who = "dusp_render_host_score_piece_buses: "

    def call(buses, sends=ones, n_buses=None, master=None, how=None, n_total=1024):
        table = (runtime.ScoreMaster * max(len(buses), 1))(*[runtime.ScoreMaster(b._h if b is not None else None, None) for b in buses])
        into = runtime.ScoreBuses(len(buses) if n_buses is None else n_buses, ctypes.addressof(table), sends.ctypes.data if sends is not None else None)
        through = runtime.ScoreMaster(master._h, None) if master is not None else None
        return L.dusp_render_host_score_piece_buses(parts, 1, 2, part_of.ctypes.data, onsets.ctypes.data, None, None, ctypes.addressof(how) if how is not None else None,
                                                    ctypes.addressof(into), ctypes.addressof(through) if through is not None else None, n_total, 0, 0, 0, out.ctypes.data, None)

    P = programs
    nan_level = ones.copy()
    nan_level[1, 0] = np.nan
    place = lambda kind, **kw: runtime.ScorePlacement(kind, kw.get("fracs"), kw.get("pans"), None, kw.get("speakers", 0), kw.get("delays"), kw.get("delays"))
    delays = np.zeros((2, 2))
    try:
        for kw, needle, status in [
            (dict(buses=[P["good"], P["no_input"]]), "a bus reads exactly one input stream (the send timeline's channel), this program has 0", -1),
            (dict(buses=[P["two_inputs"]]), "a bus reads exactly one input stream (the send timeline's channel), this program has 2", -1),
            (dict(buses=[P["wide"]]), "a bus has one output channel, this program has 2", -1),
            (dict(buses=[P["good"], P["resumable"]]), "a resumable program (DUSP_ENGINE_RESUMABLE) is not a bus", -2),
            (dict(buses=[P["elsewhere"]]), "bus 0 was built on another context", -1),
            (dict(buses=[P["good"], P["part"]]), "bus 1 is also part 0", -1),
            (dict(buses=[P["param"]]), "bus 0 has parameters but its h_params is NULL", -1),
            (dict(buses=[None]), "bus 0's program is NULL", -1),
            (dict(buses=[P["good"]], n_total=(1 << 31) + 1), "bus 0 renders channels x timeline samples, which must not exceed 2^31", -1),
            (dict(buses=[P["good"]], master=P["good"]), "bus 0 is also the master", -1),
            (dict(buses=[P["good"], P["good2"], P["good"]]), "buses 0 and 2 are the same program", -1),
            (dict(buses=[], n_buses=0), "a call has 1 .. 4 buses, not 0", -1),
            (dict(buses=[P["good"]], n_buses=5), "a call has 1 .. 4 buses, not 5", -1),
            (dict(buses=[P["good"]], sends=None), "the buses' h_sends is NULL", -1),
            (dict(buses=[P["good"], P["good2"]], sends=nan_level), "the send level of voice 0 into bus 1 is not finite", -1),
            (dict(buses=[P["good"]], how=place(runtime.PLACE_ROWS, fracs=fracs.ctypes.data)), "together with fracs, places or stereo they are refused", -2),
            (dict(buses=[P["good"]], how=place(runtime.PLACE_SPACE, speakers=2, delays=delays.ctypes.data)), "together with fracs, places or stereo they are refused", -2),
            (dict(buses=[P["good"]], how=place(runtime.PLACE_STEREO, pans=pans.ctypes.data)), "together with fracs, places or stereo they are refused", -2),
        ]:
            assert call(**kw) == status, needle
            message = L.dusp_last_error(ctx._h).decode()
            assert message.startswith(who) and needle in message, message
            assert (out == 7).all(), "a refused call wrote to h_out"
        # the strings the hosts share with the library
        assert mix.SENDS_PLACEMENT.replace("dusp-hip: ", who) in [L.dusp_last_error(ctx._h).decode()]
        assert call(buses=[P["good"], P["good2"]], sends=nan_level) == -1
        assert L.dusp_last_error(ctx._h).decode() == (mix.SENDS_NOT_FINITE % (0, 1)).replace("dusp-hip: ", who)
        assert call(buses=[], n_buses=0) == -1 and L.dusp_last_error(ctx._h).decode() == (mix.BUS_COUNT % 0).replace("dusp-hip: ", who)
        # what is a bus renders; without buses the entry is dusp_render_host_score_piece
        assert call(buses=[P["good"]]) == 0, L.dusp_last_error(ctx._h).decode()
        with_bus = out.copy()
        assert L.dusp_render_host_score_piece_buses(parts, 1, 2, part_of.ctypes.data, onsets.ctypes.data, None, None, None, None, None, 1024, 0, 0, 0, out.ctypes.data, None) == 0
        assert np.array_equal(bits(out), bits(ctx.render_score_parts([(P["part"], sv.NV, 2, two.params)], [0, 0], onsets, 1024)))
        assert (bits(with_bus) != bits(out)).sum() > 100 and not (with_bus == 7).any()
        # the device entries' own
        import torch
        buf = torch.zeros(64, dtype=torch.float32, device="cuda")
        p = buf.data_ptr()
        rows = (ctypes.c_void_p * 1)(p)
        samples, on1, one = np.array([8], dtype=np.uint32), np.zeros(1, dtype=np.int64), np.ones((1, 1), dtype=np.float32)
        send = lambda n_buses, h_sends, d_send_out: L.dusp_score_rows_send_device(ctx._h, rows, samples.ctypes.data, 1, 1, on1.ctypes.data, None, None, None, None, n_buses, h_sends, 16, None, 0,
                                                                                   p + 64, None, d_send_out, None)
        for args, needle in [((0, one.ctypes.data, p + 128), "a call has 1 .. 4 buses, not 0"), ((5, one.ctypes.data, p + 128), "a call has 1 .. 4 buses, not 5"),
                             ((1, None, p + 128), "the buses' h_sends is NULL"), ((1, one.ctypes.data, None), "NULL buffer"), ((1, one.ctypes.data, p + 130), "4-byte aligned"),
                             ((1, (one * np.inf).ctypes.data, p + 128), "the send level of voice 0 into bus 0 is not finite")]:
            assert send(*args) == -1 and needle in L.dusp_last_error(ctx._h).decode(), needle
        wets = (ctypes.c_void_p * 4)(p, p, p, p)
        for args, needle in [((p, wets, 0, 8, 0, p), "a call has 1 .. 4 buses, not 0"), ((p, wets, 5, 8, 0, p), "a call has 1 .. 4 buses, not 5"), ((None, wets, 1, 8, 0, p), "NULL buffer"),
                             ((p, wets, 1, 0, 0, p), "need 1..2^31 floats"), ((p, wets, 1, 8, 0, p + 2), "4-byte aligned")]:
            assert L.dusp_score_return_device(ctx._h, *args, None) == -1 and needle in L.dusp_last_error(ctx._h).decode(), needle
        torch.cuda.synchronize()
        assert not buf.cpu().numpy().any()  # (nothing ran)
    finally:  # (programs before their contexts, whatever failed)
        for prog in programs.values():
            prog.close()
        ctx.close()
        other.close()
