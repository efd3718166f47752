"""The master of a score or piece, on the device (dusp_render_host_score_piece): render_piece(..., master=fx) is the
CPU oracle's render of the master over what the SAME call without a master delivers — the inputs are NaN-free and a chain that starts
from +0 never holds -0, so the raw timeline the master reads and the delivered one are the same bits (mix.master_chain is the contract;
tests/test_master_host.py anchors it to the reference's one circuit).  Bit for bit, but for the Filter master: within 1e-5 of the
expected signal's largest magnitude, the project's figure for Filter graphs (tests/test_gpu_inputs.py)."""
import ctypes
import functools

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
import stereo_cases as sc
from frac_cases import layout as frac_layout
from pan_cases import pans_for
from dusp_amd import descriptor, runtime, wav
from test_piece_host import NV_SAW, bits, interleaved_voice

pytestmark = pytest.mark.gpu

RATE = sv.SAMPLE_RATE
ENGINES = {"auto": runtime.ENGINE_AUTO, "chunk": runtime.ENGINE_CHUNK, "wave": runtime.ENGINE_WAVE}
N = 13
DUR, VOICE_DUR = (sv.NT + 0.5) / RATE, (sv.NV + 0.5) / RATE
CHANNEL_ECHOES = [mc.echo_of(300.25), mc.echo_of(411.5), mc.echo_of(257.75)]  # a master a channel: one program, the delay its parameter


def voices(n=N):
    return [interleaved_voice(k) for k in range(n)]


def durations(n=N):
    return [((sv.NV if k % 2 == 0 else NV_SAW) + 0.5) / RATE for k in range(n)]


@functools.lru_cache(maxsize=None)
def plain_piece(engine):
    """the two-instrument piece without a master, as this engine renders it: what the master of the same call reads"""
    d.configure(RATE)
    onsets, _, gains = sv.layout(N)
    out = np.stack(d.render_piece(voices(), onsets, durations(), DUR, None, gains, engine=ENGINES[engine]))
    assert out.shape == (1, sv.NT) and not np.isnan(out).any() and np.abs(out).max() > 1.0
    out.setflags(write=False)
    return out


def held(name, got, want):
    """bit for bit; the Filter master within 1e-5 of the expected signal's largest magnitude"""
    assert got.dtype == np.float32 and got.shape == want.shape
    differ = int((bits(got) != bits(want)).sum())
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: %d samples differ in bits, max |err| %.3g, max |want| %.3g" % (name, differ, err, float(np.abs(want).max())))
    if name == "filter":
        assert err <= 1e-5 * float(np.abs(want).max()), err
    else:
        assert differ == 0, "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0)))


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", list(mc.MASTERS))
def test_the_seven_masters_over_a_piece_of_two_instruments(name, engine, oracle):
    fx = mc.MASTERS[name][0]
    before = plain_piece(engine)
    want = mc.oracle_master(oracle, fx, before)
    assert (bits(want) != bits(before)).sum() > 1000, "the master does nothing"
    onsets, _, gains = sv.layout(N)
    d.configure(RATE)
    got = d.render_piece(voices(), onsets, durations(), DUR, None, gains, engine=ENGINES[engine], master=fx)
    assert got.sampleRate == RATE and len(got) == 1
    held(name, np.stack(got), want)


@functools.lru_cache(maxsize=None)
def long_layout():
    rs = np.random.RandomState(10301)
    onsets = rs.randint(1, mc.LONG - 10, N).astype(np.int64)
    onsets[N // 2] = 0
    return onsets, (0.05 + 1.9 * rs.random_sample(N)).astype(np.float32)


@pytest.mark.parametrize("name", ["clip", "echo"])
def test_the_long_timeline(name, oracle):
    """10301 samples, 40 chunks and 61: the stateless Clip master's render is cut into time segments and reads its input at segment offsets"""
    fx = mc.MASTERS[name][0]
    onsets, gains = long_layout()
    d.configure(RATE)
    dur = (mc.LONG + 0.5) / RATE
    before = np.stack(d.render_piece(voices(), onsets, durations(), dur, None, gains))
    assert before.shape == (1, mc.LONG) and before[0, -2000:].any() and before[0, :2000].any()
    got = np.stack(d.render_piece(voices(), onsets, durations(), dur, None, gains, master=fx))
    held(name, got, mc.oracle_master(oracle, fx, before))
    # the same through programs of our own, to see how the master rendered: the Clip in time segments, the echo — which has state — in one
    ctx = runtime.Context(-1, RATE)
    uni, m = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(N)]), mc.unified_master(fx, 1)
    part, master = ctx.build(uni.words), ctx.build(m.words)
    try:
        mono = ctx.render_score_parts([(part, sv.NV, N, uni.params)], [0] * N, onsets, mc.LONG, None, gains)
        through = ctx.render_score_parts([(part, sv.NV, N, uni.params)], [0] * N, onsets, mc.LONG, None, gains, master=(master, m.params))
        shape = master.read_shape()
        print("the %s master over %d samples rendered as: %s" % (name, mc.LONG, shape))
        assert "compiled kernel" in shape and (" seg" in shape) == (name == "clip"), shape
        held(name, through, mc.oracle_master(oracle, fx, mono))
    finally:
        part.close()
        master.close()
        ctx.close()


def placements():
    """name -> (voices, onsets, voice durations, gains, the placement's keywords, the timeline's channels)"""
    onsets, _, gains = sv.layout(N)
    frac_onsets, fracs, frac_gains = frac_layout(N)
    mono = [sv.voice(k) for k in range(N)]
    rs = np.random.RandomState(5)
    places = rs.uniform(-3, 3, (N, 2))
    speakers = [[-1.5, 0], [1.5, 0], [0, 2]]
    return {
        "rows": ([mc.stereo_voice(k) for k in range(5)], sv.layout(5)[0], VOICE_DUR, sv.layout(5)[2], {}, 2),
        "pans": (mono, onsets, VOICE_DUR, gains, dict(pans=pans_for(N)), 2),
        "fracs_pans": (mono, frac_onsets, VOICE_DUR, frac_gains, dict(pans=pans_for(N), fracs=fracs), 2),
        "places": (mono, onsets, VOICE_DUR, gains, dict(places=places, speakers=speakers), 3),
        "stereo": (sc.voices_for(N, "in_turn"), onsets, VOICE_DUR, gains, dict(pans=sc.stereo_pans(N, "in_turn"), stereo=True), 2),
    }


@pytest.mark.parametrize("placement", ["rows", "pans", "fracs_pans", "places", "stereo"])
def test_one_master_behind_every_placement(placement, oracle):
    """the echo, with a delay of its own per channel, behind each kind of placement: channel c hears channel c alone"""
    d.configure(RATE)
    make = lambda: placements()[placement]
    _, onsets, voice_dur, gains, kw, channels = make()
    before = np.stack(d.render_piece(make()[0], onsets, voice_dur, DUR, None, gains, **kw))
    assert before.shape == (channels, sv.NT) and not np.isnan(before).any() and all(before[c].any() for c in range(channels))
    master = CHANNEL_ECHOES[:channels]
    uni = mc.unified_master(master, channels)
    assert uni.n_params == 1 and uni.params.tolist() == [[300.25, 411.5, 257.75][:channels]]
    got = np.stack(d.render_piece(make()[0], onsets, voice_dur, DUR, None, gains, master=master, **kw))
    held("echo", got, mc.oracle_master(oracle, master, before))
    # ... and one function for all channels is the same echo on each
    same = np.stack(d.render_piece(make()[0], onsets, voice_dur, DUR, None, gains, master=mc.echo, **kw))
    held("echo", same, mc.oracle_master(oracle, mc.echo, before))
    assert (bits(same[1:]) != bits(got[1:])).any()


def test_delivery_as_pcm_and_wav():
    """s16 / s24 frames and the peak of the piece behind its master: the host's quantiser over the f32 result, for every normalise mode"""
    d.configure(RATE)
    onsets, _, gains = sv.layout(N)
    args = lambda: (voices(), onsets, durations(), DUR)
    f32 = np.stack(d.render_piece(*args(), None, gains, master=mc.echo))
    peak_want = np.float32(np.abs(f32).max())
    assert peak_want > 1.0  # (normalise = 1 has something to shrink)
    for depth in (16, 24):
        for normalise in (0, 1, 2):
            res = d.render_piece_pcm(*args(), depth, normalise, None, gains, master=mc.echo)
            want, want_peak = wav.encode_frames(f32, depth, normalise)
            assert res.data.dtype == want.dtype and res.data.shape == want.shape and res.bitDepth == depth and res.numberOfChannels == 1
            assert np.array_equal(res.data.view(np.uint8), want.view(np.uint8)), (depth, normalise)
            assert np.float32(res.peak).view(np.uint32) == np.float32(want_peak).view(np.uint32) == peak_want.view(np.uint32)
    file = d.render_piece_wav(*args(), 16, 0, None, gains, master=mc.echo)
    assert file == wav.encode_wav([c for c in f32], RATE, 16) and file[:4] == b"RIFF"
    # two channels, a master a channel: the frames interleave the two masters' renders
    two = lambda: [mc.stereo_voice(k) for k in range(5)]
    on5, _, g5 = sv.layout(5)
    f32 = np.stack(d.render_piece(two(), on5, VOICE_DUR, DUR, None, g5, master=CHANNEL_ECHOES[:2]))
    res = d.render_piece_pcm(two(), on5, VOICE_DUR, DUR, 24, 2, None, g5, master=CHANNEL_ECHOES[:2])
    want, want_peak = wav.encode_frames(f32, 24, 2)
    assert res.numberOfChannels == 2 and np.array_equal(res.data.view(np.uint8), want.view(np.uint8)) and np.float32(res.peak) == np.float32(want_peak)


def test_tiles_repetition_and_a_call_without_a_master_afterwards():
    d.configure(RATE)
    onsets, _, gains = sv.layout(N)
    call = lambda **kw: np.stack(d.render_piece(voices(), onsets, durations(), DUR, None, gains, **kw))
    plain = call()
    one = call(master=mc.echo)
    # 9000 bytes: two or three voices of 3092 and 4124 bytes a tile, at least five tiles of the thirteen voices
    assert np.array_equal(bits(call(master=mc.echo, tile_bytes=9000)), bits(one)), "tiling changes the bits behind a master"
    assert np.array_equal(bits(call(master=mc.echo)), bits(one)), "the second call differs: the master did not start from its initial state"
    assert np.array_equal(bits(call()), bits(plain)), "a call without a master is not what it was before one with"
    assert (bits(one) != bits(plain)).sum() > 1000
    # the same on ONE context and ONE set of programs: the master program is reused from call to call
    ctx = runtime.Context(-1, RATE)
    uni = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(N)])
    m = mc.unified_master(mc.echo, 1)
    part, master = ctx.build(uni.words), ctx.build(m.words)
    try:
        run = lambda **kw: ctx.render_score_parts([(part, sv.NV, N, uni.params)], [0] * N, onsets, sv.NT, None, gains, **kw)
        before = run()
        first = run(master=(master, m.params))
        assert np.array_equal(bits(run(master=(master, m.params), tile_bytes=7000)), bits(first)) and np.array_equal(bits(run()), bits(before))
        assert (bits(first) != bits(before)).sum() > 1000
        with pytest.raises(runtime.DuspHipError, match="last render was a mix"):
            master.state(0)
    finally:
        part.close()
        master.close()
        ctx.close()


def test_render_score_with_a_master_is_render_piece_of_one_structure(oracle):
    d.configure(RATE)
    onsets, lengths, gains = sv.layout(N)
    mono = lambda: [sv.voice(k) for k in range(N)]
    want = np.stack(d.render_piece(mono(), onsets, VOICE_DUR, DUR, lengths, gains, master=mc.allpass))
    got = d.render_score(mono(), onsets, VOICE_DUR, DUR, lengths, gains, master=mc.allpass)
    assert got.sampleRate == RATE and len(got) == 1 and np.array_equal(bits(np.stack(got)), bits(want))
    # ... and the oracle's master over the score without one, which goes the contiguous way
    plain = np.stack(d.render_score(mono(), onsets, VOICE_DUR, DUR, lengths, gains))
    held("allpass", want, mc.oracle_master(oracle, mc.allpass, plain))
    assert len(d.render_score(mono(), onsets, VOICE_DUR, 0, master=mc.allpass)) == 0
    pcm = d.render_score_pcm(mono(), onsets, VOICE_DUR, DUR, 16, 1, lengths, gains, master=mc.allpass)
    assert np.array_equal(pcm.data, wav.encode_frames(want, 16, 1)[0])


# ---- the C entry, through ctypes -------------------------------------------------------------------------------------------------------

def test_the_c_entry_refuses_what_is_no_master_before_anything_renders():
    d.configure(RATE)
    L = runtime.load()
    ctx, other = runtime.Context(-1, RATE), runtime.Context(-1, RATE)
    two = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(2)])
    build = lambda c, outlet, engine=runtime.ENGINE_AUTO: c.build(descriptor.extract(outlet).words, engine)
    echo = mc.unified_master(CHANNEL_ECHOES[:1], 1)
    with_param = mc.unified_master(CHANNEL_ECHOES[:2], 2)  # (a program with one parameter: the delay)
    programs = dict(part=ctx.build(two.words), good=ctx.build(echo.words), no_input=build(ctx, sv.voice(5)),
                    two_inputs=build(ctx, d.Sum(d.MasterInput(), d.HostSource(np.zeros(4)))), wide=build(ctx, d.Pan(d.MasterInput(), 0.25)),
                    resumable=ctx.build(echo.words, runtime.ENGINE_AUTO | runtime.ENGINE_RESUMABLE), elsewhere=other.build(echo.words), param=ctx.build(with_param.words))
    assert programs["param"].n_params == 1 and programs["wide"].n_out_channels == 2 and programs["two_inputs"].n_inputs == 2
    parts = (runtime.ScorePart * 1)(runtime.ScorePart(programs["part"]._h, 2, sv.NV, two.params.ctypes.data))
    part_of, onsets = np.zeros(2, dtype=np.uint32), np.array([0, 40], dtype=np.int64)
    out = np.full((1, 1024), 7, dtype=np.float32)

    def call(master, h_params=None, n_total=1024):
        through = runtime.ScoreMaster(master._h, h_params)
        return L.dusp_render_host_score_piece(parts, 1, 2, part_of.ctypes.data, onsets.ctypes.data, None, None, None, ctypes.addressof(through), n_total, 0, 0, 0, out.ctypes.data, None)

    try:
        for master, n_total, needle, status in [
            (programs["no_input"], 1024, "a master reads exactly one input stream (the timeline's channel), this program has 0", -1),
            (programs["two_inputs"], 1024, "a master reads exactly one input stream (the timeline's channel), this program has 2", -1),
            (programs["wide"], 1024, "a master has one output channel, this program has 2", -1),
            (programs["resumable"], 1024, "a resumable program (DUSP_ENGINE_RESUMABLE) is not a master", -2),
            (programs["elsewhere"], 1024, "the master was built on another context", -1),
            (programs["part"], 1024, "the master is also part 0", -1),
            (programs["param"], 1024, "the master has parameters but its h_params is NULL", -1),
            (programs["good"], (1 << 31) + 1, "the master renders channels x timeline samples, which must not exceed 2^31", -1),
        ]:
            assert call(master, None, n_total) == status, needle
            message = L.dusp_last_error(ctx._h).decode()
            assert message.startswith("dusp_render_host_score_piece: ") and needle in message, message
            assert (out == 7).all(), "a refused call wrote to h_out"
        # what is a master renders, and the entry without one is dusp_render_host_score_parts
        assert call(programs["good"]) == 0, L.dusp_last_error(ctx._h).decode()
        with_master = out.copy()
        assert L.dusp_render_host_score_piece(parts, 1, 2, part_of.ctypes.data, onsets.ctypes.data, None, None, None, None, 1024, 0, 0, 0, out.ctypes.data, None) == 0
        assert np.array_equal(bits(out), bits(ctx.render_score_parts([(programs["part"], sv.NV, 2, two.params)], [0, 0], onsets, 1024)))
        assert (bits(with_master) != bits(out)).sum() > 100 and not (with_master == 7).any()  # (the echo is heard from sample 301 or a chunk later)
        bad = runtime.ScorePlacement(9, None, None, None, 0, None, None)
        assert L.dusp_render_host_score_piece(parts, 1, 2, part_of.ctypes.data, onsets.ctypes.data, None, None, ctypes.addressof(bad), None, 1024, 0, 0, 0, out.ctypes.data, None) == -1
        assert "the placement's kind must be" in L.dusp_last_error(ctx._h).decode()
    finally:  # (programs before their contexts, whatever failed)
        for prog in programs.values():
            prog.close()
        ctx.close()
        other.close()
