"""Tracks on the CPU.  The contract is: today's chain over every destination's voices (the direct voices, every
track's), mix.master_chain per track that has a circuit, mix.track_mix, then the buses and the master as they stand.  The anchor test
holds it to the reference's ONE circuit — a tree: Sum.many([Sum.many(direct), Multiply(fx_0(Sum.many(track 0)), f_0), ...]) — on the
CPU oracle and asserts what is found, the table of DESIGN.md 6.16.  Then track_mix against a plain loop over planted values, the
kernel's text on the host under sanitizers, and the Python surface without a device."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
import track_cases as tc
from dusp_amd import descriptor, mix, render
from test_piece_host import ROOT, SANITIZE, bits, same

PAIRS = {"clip+echo": ("clip", "echo"), "comb+allpass": ("comb", "allpass"), "lowpass+lowpass": ("lowpass", "lowpass")}
# DESIGN.md 6.16's anchor table: (tracks, voices, direct voices?, faders?, a master behind the tree) -> is the contract the one circuit
# bit for bit?  What was found is asserted, equal or not, so that the table cannot rot: every case tried is equal, the Filter tracks too.
ANCHOR = {(pair, n, direct, fade, None): True for pair in ("clip+echo", "comb+allpass") for n in (5, 13) for direct in (True, False) for fade in (False, True)}
ANCHOR.update({("lowpass+lowpass", 13, True, True, None): True, ("clip+echo", 13, True, True, "allpass"): True, ("comb+allpass", 5, False, False, "echo"): True})


@functools.lru_cache(maxsize=None)
def voice_rows(n, oracle):
    d.configure(sv.SAMPLE_RATE)
    uni = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(n)])
    rows = tuple(np.asarray(r, dtype=np.float32) for r in oracle.render_instances(uni.words, sv.NV, uni.params, n, range(n)))
    for r in rows:
        r.setflags(write=False)
    return rows


@pytest.mark.parametrize("case", list(ANCHOR), ids=lambda c: "-".join(str(x) for x in c))
def test_the_contract_against_the_one_circuit(case, oracle):
    pair, n, direct, fade, master = case
    fxs = [tc.TRACKS[name] for name in PAIRS[pair]]
    onsets, _, gains = sv.layout(n)
    of = tc.track_of(n, 2, direct)
    assert (of == -1).any() == direct and all((of == g).any() for g in range(2))
    f = tc.faders(2) if fade else None
    d.configure(sv.SAMPLE_RATE)
    tree = tc.one_circuit(fxs, [sv.voice(k) for k in range(n)], onsets, gains, of, f)
    if master is not None:
        tree = tc.TRACKS[master](tree)
    want = np.asarray(oracle.render(descriptor.extract(tree).words, sv.NT), dtype=np.float32)
    got = tc.expected(oracle, list(voice_rows(n, oracle)), onsets, sv.NT, fxs, of, 1, f, gains=gains, master=None if master is None else tc.TRACKS[master])
    plain = mix.score_chain_rows(list(voice_rows(n, oracle)), onsets, sv.NT, None, gains)
    assert got.shape == want.shape == (1, sv.NT) and got.dtype == np.float32
    assert (bits(got) != bits(plain)).sum() > 500  # (the tracks are heard)
    equal = bool(np.array_equal(bits(got), bits(want)))
    print("%s: %d samples differ in bits, max |err| %.3g" % (case, int((bits(got) != bits(want)).sum()), float(np.abs(got.astype(np.float64) - want).max())))
    assert equal == ANCHOR[case]


# ---- track_mix ----------------------------------------------------------------------------------------------------------------------------

def planted(shape, seed):
    rs = np.random.RandomState(seed)
    a = (rs.standard_normal(shape) * 10.0 ** rs.randint(-3, 4, shape)).astype(np.float32)
    flat = a.reshape(-1)
    for j, v in enumerate([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -5e-39, np.finfo(np.float32).max]):
        flat[(7 * j + 3 + seed) % flat.size] = v
    return a


def loop_track_mix(direct, ys, faders, sends):
    """the contract, float by float"""
    f32 = np.float32
    out = np.empty_like(direct)
    n_buses = 0 if sends is None else len(sends)
    feeds = np.zeros((n_buses,) + direct.shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        for at in np.ndindex(*direct.shape):
            acc, feed = f32(direct[at]), [f32(0)] * n_buses
            for g, y in enumerate(ys):
                term = f32(y[at]) if faders is None else f32(f32(y[at]) * f32(faders[g]))
                acc = f32(acc + term)
                for b in range(n_buses):
                    feed[b] = f32(feed[b] + f32(term * f32(sends[b][g])))
            out[at] = acc
            for b in range(n_buses):
                feeds[(b,) + at] = feed[b]
    return out, feeds


@pytest.mark.parametrize("n_buses", [0, 1, 4])
@pytest.mark.parametrize("with_faders", [False, True])
@pytest.mark.parametrize("n_tracks", [1, 3, 8])
def test_track_mix_against_a_plain_loop(n_tracks, with_faders, n_buses):
    shape = (2, 131)
    direct, ys = planted(shape, 1), [planted(shape, 10 + g) for g in range(n_tracks)]
    faders = [0.0, -0.0, 1.0, -0.75, 1e-30, 3e20, 0.6, 2.0][:n_tracks] if with_faders else None
    sends = None if not n_buses else np.array([[0.0, -0.0, 1.0, -0.5, 1e-30, 3e20, 0.25, 1.5][(b + g) % 8] for b in range(n_buses) for g in range(n_tracks)], dtype=np.float32).reshape(n_buses, n_tracks)
    got, feeds = mix.track_mix(direct, ys, faders, sends)
    want, want_feeds = loop_track_mix(direct, ys, faders, sends)
    assert got.dtype == feeds.dtype == np.float32 and feeds.shape == (n_buses,) + shape
    assert same(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    assert same(feeds, want_feeds) and np.array_equal(np.signbit(feeds), np.signbit(want_feeds))
    assert np.isnan(got).any() and np.isinf(got).any()  # (raw: nothing is made 0)


def test_raw_values_reach_a_track_circuit_and_pass_a_track_without_one(oracle):
    """a track's circuit hears its raw sub-mix — NaN and Inf as the chain left them — and applies `|| 0` at its own copy-out; a track
    WITHOUT a circuit passes its raw sub-mix on, NaN included, and a level of 0 over it poisons the feed"""
    x = np.array([[1.0, np.nan, -2.0, np.inf, 3.0, -0.0]], dtype=np.float32)
    rows, onsets = [x, x], [0, 8]
    heard = []

    def spy(c, samples):
        heard.append(samples.copy())
        return np.where(np.isnan(samples), np.float32(0), samples)

    sub = tc.sub_chain(rows, onsets, 16, [0], 1)
    assert np.isnan(sub[0, 1]) and np.isinf(sub[0, 3]) and not np.signbit(sub[0, 5])  # (a chain from +0 holds no -0: +0 + -0 is +0)
    y = mix.master_chain(sub, spy)
    assert same(heard[0], sub[0]) and not np.isnan(y).any()
    bare = tc.sub_chain(rows, onsets, 16, [1], 1)
    out, feeds = mix.track_mix(np.zeros((1, 16), dtype=np.float32), [y, bare], None, [[1.0, 0.0]])
    assert out[0, 1] == 0 and np.isnan(out[0, 9]), "a track without a circuit passes a NaN on; one with a circuit has none to pass"
    assert np.isnan(feeds[0, 0, 9]) and np.isnan(feeds[0, 0, 11]) and feeds[0, 0, 0] == 1, "a level of 0 over a NaN (or Inf) track poisons the feed"
    assert np.signbit(mix.track_mix(np.full((1, 1), -0.0, dtype=np.float32), [np.array([[2.0]], dtype=np.float32)], [-0.0])[0][0, 0])  # (-0 + -0)
    # the clip over a planted sub-mix through the oracle: the same, end to end
    d.configure(sv.SAMPLE_RATE)
    want = tc.expected(oracle, rows, onsets, 16, [mc.clip, None], [0, 1])
    assert want[0, 1] == 0 and want[0, 9] == 0 and want[0, 8] == 1  # (`|| 0` at the delivery)
    with pytest.raises(ValueError, match="the output of track 1 must have shape"):
        mix.track_mix(sub, [sub, sub[:, :3]])
    with pytest.raises(ValueError, match="the raw timeline is float32"):
        mix.track_mix(sub.astype(np.float64), [sub])


# ---- the kernel's text, under sanitizers ------------------------------------------------------------------------------------------------

def test_score_tracks_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/score_tracks_engine.hip itself, compiled for the host with its lanes run one after the other, every buffer a heap
    allocation of exactly its size, under AddressSanitizer and UBSan, against a brute-force chain
    (tests/native/score_tracks_kernel_check.cpp lists what it covers)."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "score_tracks_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub"), "-x", "c++",
                           os.path.join(native, "score_tracks_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 8000 and rep["wide"] > 1000 and rep["narrow"] > 1000 and rep["strided"] == 2, rep


# ---- the Python surface, without a device ------------------------------------------------------------------------------------------------

CALLS = (d.render_piece, d.render_score, d.render_piece_pcm, d.render_score_pcm, d.render_piece_wav, d.render_score_wav)


def voices(n=3):
    return [sv.voice(k) for k in range(n)]


def test_check_tracks():
    of, f, s = mix.check_tracks(3, 2, [0, -1, 1], [0.5, 2], [[0, 1], [1, 0.25]], 2)
    assert of.dtype == np.int32 and of.tolist() == [0, -1, 1] and of.flags.c_contiguous
    assert f.dtype == np.float32 and f.tolist() == [0.5, 2] and s.dtype == np.float32 and s.shape == (2, 2) and s.flags.c_contiguous
    assert mix.check_tracks(3, 2, np.array([0.0, -1.0, 1.0]), None, [0.5, 1], 1)[2].shape == (1, 2)
    assert mix.check_tracks(3, None, None) == (None, None, None)
    assert mix.check_tracks(0, 1, [])[0].shape == (0,)  # (a track with no voices is allowed)


@pytest.mark.parametrize("call", CALLS, ids=lambda c: c.__name__)
def test_what_does_not_go_with_tracks_is_refused_by_string(call):
    d.configure(sv.SAMPLE_RATE)
    of, two = [0, -1, 0], [mc.clip, None]
    for kw, message in (
            (dict(track_of=of), mix.TRACKS_TRACK_OF_ALONE),
            (dict(faders=[1]), mix.TRACKS_NEED_TRACKS % "faders"),
            (dict(track_sends=[[1]]), mix.TRACKS_NEED_TRACKS % "track_sends"),
            (dict(tracks=[mc.clip]), mix.TRACKS_WITHOUT_TRACK_OF),
            (dict(tracks=[], track_of=of), mix.TRACKS_COUNT % 0),
            (dict(tracks=[None] * 9, track_of=of), mix.TRACKS_COUNT % 9),
            (dict(tracks=mc.clip, track_of=of), mix.TRACKS_COUNT % 0),
            (dict(tracks=two, track_of=[0, 1]), mix.TRACKS_TRACK_OF_SHAPE % 3),
            (dict(tracks=two, track_of=[0, 0.5, 1]), mix.TRACKS_TRACK_OF_SHAPE % 3),
            (dict(tracks=two, track_of=[0, 2, 1]), mix.TRACKS_TRACK_OF_RANGE % (1, 2, 2, 1)),
            (dict(tracks=two, track_of=[0, 1, -2]), mix.TRACKS_TRACK_OF_RANGE % (2, -2, 2, 1)),
            (dict(tracks=two, track_of=of, faders=[1]), mix.TRACKS_FADERS_SHAPE % 2),
            (dict(tracks=two, track_of=of, faders=[1, np.nan]), mix.TRACKS_FADER_NOT_FINITE % 1),
            (dict(tracks=two, track_of=of, faders=[1e39, 1]), mix.TRACKS_FADER_NOT_FINITE % 0),
            (dict(tracks=two, track_of=of, track_sends=[[1, 1]]), mix.TRACKS_SENDS_WITHOUT_BUSES),
            (dict(tracks=two, track_of=of, buses=[mc.echo]), mix.TRACKS_BUSES_WITHOUT_SENDS),
            (dict(tracks=two, track_of=of, buses=[mc.echo], sends=[1, 1, 1]), mix.TRACKS_WITH_SENDS),
            (dict(tracks=two, track_of=of, buses=[mc.echo], sends=[1, 1, 1], track_sends=[[1, 1]]), mix.TRACKS_WITH_SENDS),
            (dict(tracks=two, track_of=of, buses=[], track_sends=[[1, 1]]), mix.BUS_COUNT % 0),
            (dict(tracks=two, track_of=of, buses=[mc.echo] * 5, track_sends=np.ones((5, 2))), mix.BUS_COUNT % 5),
            (dict(tracks=two, track_of=of, buses=[mc.echo], track_sends=[[1, 1, 1]]), mix.TRACKS_SENDS_SHAPE % (1, 2)),
            (dict(tracks=two, track_of=of, buses=[mc.echo, mc.comb], track_sends=[1, 1]), mix.TRACKS_SENDS_SHAPE % (2, 2)),
            (dict(tracks=two, track_of=of, buses=[mc.echo, mc.comb], track_sends=[[1, 1], [np.inf, 1]]), mix.TRACKS_LEVEL_NOT_FINITE % (0, 1))):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0, **kw)
        assert str(e.value) == message, kw
    # with tracks the buses are fed by the tracks: every placement goes with them
    for kw in (dict(fracs=[0, 0.5, 0]), dict(places=[[0, 0], [1, 1], [2, 0]], speakers=[[-1, 0], [1, 0]]), dict(stereo=True)):
        res = call(voices(), [1, 2, 3], 0.01, 0, tracks=two, track_of=of, buses=[mc.echo], track_sends=[1, 0], **kw)
        assert isinstance(res, bytes) or len(getattr(res, "data", res)) == 0


def scheduled(x):
    u = mc.clip(x)
    u.schedule(0.01, lambda unit: None)
    return u


TRACK_REFUSALS = {
    "notCallable": (lambda: 5, 1, mix.TRACK_NOT_CALLABLE % 1),
    "emptyList": (lambda: [], 1, mix.TRACK_NOT_CALLABLE % 1),
    "count": (lambda: [mc.echo], 2, mix.TRACK_CIRCUITS % (1, 1, 2)),
    "noInput": (lambda: (lambda x: sv.voice(0)), 1, mix.TRACK_ONE_INPUT % (1, 0, 0)),
    "hostSource": (lambda: (lambda x: d.Sum(x, d.HostSource(np.zeros(8)))), 1, mix.TRACK_HOST_SOURCE % (1, 0)),
    "events": (lambda: scheduled, 1, mix.TRACK_EVENTS % (1, 0)),
    "channels": (lambda: (lambda x: d.Pan(x, 0.25)), 1, mix.TRACK_CHANNELS % (1, 0, 2)),
    "notIsomorphic": (lambda: [mc.echo, mc.clip], 2, mix.TRACK_NOT_ISOMORPHIC % (1, 1)),
}


@pytest.mark.parametrize("case", list(TRACK_REFUSALS))
def test_what_is_no_track_is_refused_by_string(case):
    """a track's circuit is held to a bus's rules, in a bus's words with "track g" for the noun; track 1 of two is the one at fault"""
    track, channels, message = TRACK_REFUSALS[case]
    d.configure(sv.SAMPLE_RATE)
    with pytest.raises(descriptor.DuspError) as e:
        render.track_programs([None, track()], channels, sv.SAMPLE_RATE)
    assert str(e.value) == message and message.startswith("dusp-hip: ") and "track 1" in message
    kw = dict(pans=[0, 0.5, -0.5]) if channels == 2 else {}
    for call in CALLS:
        with pytest.raises(descriptor.DuspError) as e:
            call(voices(), [0, 1, 2], 0.01, 0, tracks=[mc.echo, track()], track_of=[0, 1, -1], **kw)
        assert str(e.value) == message, call.__name__
    d.configure(44100)
    with pytest.raises(descriptor.DuspError) as e:
        render.track_programs([None, None, mc.clip], 1, 48000)
    assert str(e.value) == mix.TRACK_RATE % (2, 44100, 48000)
    d.configure(sv.SAMPLE_RATE)


def test_tracks_with_isomorphic_circuits_are_one_program():
    d.configure(sv.SAMPLE_RATE)
    groups = render.track_programs([mc.echo_of(300.25), mc.clip, None, mc.echo_of(411.5), [mc.echo_of(100.5)], mc.clip], 1, sv.SAMPLE_RATE)
    assert [which for _, which in groups] == [[0, 3, 4], [1, 5]]
    echoes, clips = groups[0][0], groups[1][0]
    assert echoes.n_instances == 3 and echoes.n_params == 1 and echoes.params.tolist() == [[300.25, 411.5, 100.5]]
    assert clips.n_instances == 2 and clips.n_params == 0
    # two channels: the instances are (track, channel), a column each
    groups = render.track_programs([[mc.echo_of(300.25), mc.echo_of(411.5)], mc.echo_of(100.5)], 2, sv.SAMPLE_RATE)
    assert len(groups) == 1 and groups[0][1] == [0, 1] and groups[0][0].params.tolist() == [[300.25, 411.5, 100.5, 100.5]]
    assert render.track_programs([None, None], 2, sv.SAMPLE_RATE) == []


def test_tracks_travel_with_the_placement_to_the_piece():
    d.configure(sv.SAMPLE_RATE)
    placing = render._placing(None, None, None, None, -3, None, False)
    assert placing["tracks"] is None and placing["track_of"] is None
    *_, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, placing)
    assert place.tracks is None and "tracks" not in place.keywords()
    for kw, want in ((dict(), 1), (dict(pans=[0, 0.5, -0.5]), 2)):
        placing = render._placing(kw.get("pans"), None, None, None, -3, None, False, mc.clip, [mc.echo], None, [mc.echo_of(200.5), None, mc.echo], [2, -1, 0], [1, 0.5, 2], [[1, 0, 0.5]])
        *_, channels, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, placing)
        n_tracks, of, groups, f, s = place.tracks
        assert channels == want and n_tracks == 3 and of.dtype == np.int32 and of.tolist() == [2, -1, 0] and f.tolist() == [1, 0.5, 2] and s.tolist() == [[1, 0, 0.5]]
        assert len(groups) == 1 and groups[0][1] == [0, 2] and groups[0][0].n_instances == 2 * want
        assert place.sends is None and len(place.buses) == 1 and place.master.n_instances == want
    # every other refusal of the call comes first; the master's before the tracks', the tracks' before the buses'
    with pytest.raises(ValueError, match="pans must have shape"):
        d.render_piece(voices(), [0, 1, 2], 0.01, 0.05, pans=[0], tracks=[5], track_of=[0, 0, 0])
    with pytest.raises(descriptor.DuspError) as e:
        d.render_piece(voices(), [0, 1, 2], 0.01, 0.05, master=5, tracks=[5], track_of=[0, 0, 0])
    assert str(e.value) == mix.MASTER_NOT_CALLABLE
    with pytest.raises(descriptor.DuspError) as e:
        d.render_piece(voices(), [0, 1, 2], 0.01, 0.05, tracks=[5], track_of=[0, 0, 0], buses=[5], track_sends=[1])
    assert str(e.value) == mix.TRACK_NOT_CALLABLE % 0
    # a score with tracks goes the piece's way, as one part
    with pytest.raises(descriptor.DuspError, match="the voices of a score are isomorphic circuits"):
        d.render_score([sv.voice(0), mc.stereo_voice(1)], [0, 1], 0.01, 0, tracks=[mc.echo], track_of=[0, -1])
    assert len(d.render_score(voices(), [0, 1, 2], 0.01, 0, tracks=[mc.echo, None], track_of=[0, 1, -1], faders=[1, 0.5])) == 0
    assert d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, tracks=[None], track_of=[0, 0, 0]).data.shape == (0, 1)
