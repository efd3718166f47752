"""Stems without a device: the contract mix.stems / mix.track_terms against a plain loop; the property that makes them
stems — without a master and without NaN they add up, left-deep in f32, to the mix bit for bit — over the thirteen-voice cases of
track_cases and send_cases, and its counter-example, a NaN through a fader group; wav.encode_stems against the quantiser a signal with
the common gain put in by hand; the refusal string and the routing of stems=; and the text of the two new kernels on the host under
sanitizers (tests/native/score_stems_kernel_check.cpp)."""
import json
import os
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
import send_cases as sc
import stem_cases as stc
import track_cases as tc
from dusp_amd import descriptor, mix, render, wav
from pan_cases import pans_for
from test_piece_host import ROOT, SANITIZE, bits, oracle_rows, same
from test_tracks_host import planted

N = 13


def or0(x):
    return np.float32(0) if (x != x or x == 0) else np.float32(x)


# ---- the contract against a plain loop --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_tracks, with_faders, n_buses", [(0, False, 0), (1, True, 0), (3, False, 2), (8, True, 4), (0, False, 3)])
def test_stems_and_track_terms_against_a_plain_loop(n_tracks, with_faders, n_buses):
    shape = (2, 131)
    direct, ys = planted(shape, 1), [planted(shape, 10 + g) for g in range(n_tracks)]
    wets, out = [planted(shape, 30 + b) for b in range(n_buses)], planted(shape, 50)
    faders = [0.0, -0.0, 1.0, -0.75, 1e-30, 3e20, 0.6, 2.0][:n_tracks] if with_faders else None
    terms = mix.track_terms(ys, faders)
    assert len(terms) == n_tracks and all(t.dtype == np.float32 for t in terms)
    with np.errstate(all="ignore"):
        for g, (t, y) in enumerate(zip(terms, ys)):
            want = np.array([np.float32(v) if faders is None else np.float32(np.float32(v) * np.float32(faders[g])) for v in y.reshape(-1)], dtype=np.float32).reshape(shape)
            assert same(t, want) and np.array_equal(np.signbit(t), np.signbit(want))
    if n_tracks:  # track_mix is what it was, and it adds these terms
        acc = direct.copy()
        with np.errstate(all="ignore"):
            for t in terms:
                acc = acc + t
        assert same(mix.track_mix(direct, ys, faders)[0], acc)
    got = mix.stems(direct, terms, wets, out)
    assert got.dtype == np.float32 and got.shape == (1 + n_tracks + n_buses + 1,) + shape
    assert mix.stem_names(n_tracks, n_buses) == ["direct"] + ["track%d" % g for g in range(n_tracks)] + ["bus%d" % b for b in range(n_buses)] + ["mix"]
    for s, raw in enumerate([direct] + terms):
        want = np.array([or0(v) for v in raw.reshape(-1)], dtype=np.float32).reshape(shape)
        assert np.array_equal(bits(got[s]), bits(want)), "slot %d is not `|| 0`" % s
        assert not np.isnan(got[s]).any() and not (np.signbit(got[s]) & (got[s] == 0)).any() and np.array_equal(np.isinf(got[s]), np.isinf(raw))  # (Inf stays)
    assert np.isinf(got[0]).any()
    for b, wet in enumerate(wets):  # (a bus's output is kept as its copy-out left it)
        assert same(got[1 + n_tracks + b], wet) and np.array_equal(np.signbit(got[1 + n_tracks + b]), np.signbit(wet))
    assert same(got[-1], out)
    with pytest.raises(ValueError, match="the output of track 0 must have shape"):
        mix.stems(direct, [direct[:, :3]], [], out)
    with pytest.raises(ValueError, match="the output of bus 0 must have shape"):
        mix.stems(direct, [], [direct[:1]], out)
    with pytest.raises(ValueError, match="the raw timeline is float32"):
        mix.stems(direct.astype(np.float64), [], [], out)
    with pytest.raises(ValueError) as e:
        mix.track_terms([direct, direct], [1.0, np.nan])
    assert str(e.value) == mix.TRACKS_FADER_NOT_FINITE % 1


# ---- the property that makes these stems ------------------------------------------------------------------------------------------------

CASES = {
    "clip+echo, direct voices": dict(fxs=("clip", "echo")),
    "clip+echo, faders": dict(fxs=("clip", "echo"), fade=True),
    "clip, fader group, silent echo": dict(fxs=("clip", None, "echo"), fade=True, n_of=2),
    "tracks into two buses": dict(fxs=("clip", "echo", None), fade=True, buses=("echo", "comb")),
    "eight fader groups": dict(fxs=(None,) * 8, fade=True),
    "per-note sends": dict(buses=("echo",), sends=True),
    "per-note sends, pans, two buses": dict(buses=("echo", "comb"), sends=True, pans=True),
    "one timeline": dict(),
}


def case_stack(name, oracle, master=None):
    c = CASES[name]
    onsets, _, gains = sv.layout(N)
    rows = list(oracle_rows(N, oracle))
    buses = [tc.TRACKS[b] for b in c.get("buses", ())] or None
    master = None if master is None else tc.TRACKS[master]
    if "fxs" in c:
        fxs = [None if f is None else tc.TRACKS[f] for f in c["fxs"]]
        T = len(fxs)
        return stc.expected(oracle, rows, onsets, sv.NT, fxs, tc.track_of(N, c.get("n_of", T)), 1, tc.faders(T) if c.get("fade") else None, gains=gains, buses=buses,
                            track_sends=tc.levels(len(buses), T) if buses else None, master=master)
    if c.get("pans"):
        d.configure(sv.SAMPLE_RATE)
        mono = tc.oracle_voice_rows(oracle, [sv.voice(k) for k in range(N)], [sv.NV] * N)
        return stc.expected(oracle, mono, onsets, sv.NT, channels=2, gains=gains, buses=buses, sends=sc.levels(N, len(buses)), master=master, pans=pans_for(N))
    return stc.expected(oracle, rows, onsets, sv.NT, gains=gains, buses=buses, sends=sc.levels(N, len(buses)) if buses else None, master=master)


@pytest.mark.parametrize("name", list(CASES))
def test_the_stems_add_up_to_the_mix_bit_for_bit(name, oracle):
    stack = case_stack(name, oracle)
    c = CASES[name]
    assert stack.shape[0] == 1 + len(c.get("fxs", ())) + len(c.get("buses", ())) + 1 and stack.shape[2] == sv.NT
    assert not np.isnan(stack).any() and np.abs(stack[-1]).max() > 0.1
    total = mix.stems_sum(stack)
    assert np.array_equal(bits(total), bits(stack[-1])), "%d samples of the summed stems are not the mix" % int((bits(total) != bits(stack[-1])).sum())
    if stack.shape[0] > 2:  # (every stem but the silent echo's is heard, and no stem is the mix)
        silent = [s for s in range(stack.shape[0] - 1) if not stack[s].any()]
        assert silent == ([3] if "silent" in name else []), silent
        assert all((bits(stack[s]) != bits(stack[-1])).sum() > 500 for s in range(stack.shape[0] - 1))
    else:
        assert np.array_equal(bits(stack[0]), bits(stack[1]))  # S = 1: direct is the mix


def test_behind_a_master_the_stems_are_in_front_of_it(oracle):
    plain, mastered = case_stack("clip+echo, faders", oracle), case_stack("clip+echo, faders", oracle, "allpass")
    assert np.array_equal(bits(plain[:-1]), bits(mastered[:-1])) and (bits(plain[-1]) != bits(mastered[-1])).sum() > 1000
    assert (bits(mix.stems_sum(mastered)) != bits(mastered[-1])).sum() > 1000  # (they add up to what the master hears, not to what it makes of it)


def test_a_nan_through_a_fader_group_breaks_the_sum():
    """the counter-example, pinned: a fader group passes a NaN of its voices on, so the mix is NaN there and leaves as 0; the group's
    stem is 0 there too, but the other stems add up to the direct voice's sample"""
    x = np.array([[1.0, np.nan, -2.0, 0.5, 3.0, -0.0]], dtype=np.float32)
    clean = np.array([[0.25, 0.5, 0.75, 1.0, 1.25, 1.5]], dtype=np.float32)
    rows, onsets, of = [x, clean], [0, 0], [0, -1]
    direct = tc.sub_chain(rows, onsets, 8, [1], 1)
    ys = [tc.sub_chain(rows, onsets, 8, [0], 1)]
    f = np.array([0.5], dtype=np.float32)
    out = mix.bus_return(mix.track_mix(direct, ys, f)[0], [])
    stack = mix.stems(direct, mix.track_terms(ys, f), [], out)
    assert np.isnan(ys[0][0, 1]) and stack[1][0, 1] == 0 and stack[2][0, 1] == 0, "the stem is 0 there and the mix is 0 there"
    total = mix.stems_sum(stack)
    assert total[0, 1] == np.float32(0.5) != stack[2][0, 1], "but the sum of the other stems is not"
    others = np.arange(8) != 1
    assert np.array_equal(bits(total[:, others]), bits(stack[2][:, others]))
    assert of == [0, -1]


# ---- one gain --------------------------------------------------------------------------------------------------------------------------

def loud_stems(n=257, channels=2):
    """two tracks at faders +1 and -1 over nearly the same signal: each stem is about 1.6 at its peak, the mix a hundredth of that"""
    rs = np.random.RandomState(3)
    x = (1.6 * np.sin(np.arange(channels * n) * 0.37).reshape(channels, n)).astype(np.float32)
    y = (x * np.float32(1.01) + 1e-3 * rs.standard_normal((channels, n))).astype(np.float32)
    direct = np.zeros((channels, n), dtype=np.float32)
    f = np.array([1.0, -1.0], dtype=np.float32)
    out = mix.bus_return(mix.track_mix(direct, [x, y], f)[0], [])
    return mix.stems(direct, mix.track_terms([x, y], f), [], out)


@pytest.mark.parametrize("normalise", [0, 1, 2])
@pytest.mark.parametrize("depth", [16, 24, 32])
def test_encode_stems_is_the_quantiser_a_signal_under_the_common_gain(depth, normalise):
    stack = loud_stems()
    own = np.array([wav.peak(x) for x in stack], dtype=np.float32)
    assert own[1] > 1.5 and own[2] > own[1] > 50 * own[3] and own[0] == 0, "the loudest signal is a stem, not the mix"
    frames, peaks = wav.encode_stems(stack, depth, normalise)
    assert peaks.dtype == np.float32 and np.array_equal(bits(peaks), bits(own))
    common = wav.common_peak(peaks)
    assert bits(common) == bits(own[2])
    g = wav.gain(common, normalise)
    assert (g == 1.0) == (normalise == 0) and (normalise == 0 or g == np.float64(1.0) / np.float64(own[2]))
    for s, x in enumerate(stack):  # encode_frames' own steps, signal by signal, with the common gain put in by hand
        want = wav.scale_f32(x.T, g) if depth == 32 else wav.pack(wav.quantise(x.T, g, depth), depth)
        assert frames[s].dtype == want.dtype and np.array_equal(np.ascontiguousarray(frames[s]).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), (s, depth, normalise)
        if normalise == 0:
            assert np.array_equal(frames[s].view(np.uint8), wav.encode_frames(x, depth, 0)[0].view(np.uint8))
    if normalise and depth != 32:  # a gain a signal would have blown the mix up to full scale; under the common gain the files still add up
        q = lambda s: wav.quantise(stack[s].T, g, depth).astype(np.int64)
        assert np.abs(q(3)).max() < 0.02 * wav.SCALE[depth] and np.abs(q(1)).max() > 0.9 * wav.SCALE[depth]
        assert np.abs(q(0) + q(1) + q(2) - q(3)).max() <= 2, "the delivered stems add up to the delivered mix within the quantiser's rounding"
        assert np.abs(wav.quantise(stack[3].T, wav.gain(own[3], normalise), depth)).max() > 0.5 * wav.SCALE[depth] or normalise == 1
    # a NaN peak wins and leaves the gain at 1, as one signal's does
    poisoned = stack.copy()
    poisoned[1, 0, 5] = np.nan
    _, p = wav.encode_stems(poisoned, depth, normalise)
    assert np.isnan(p[1]) and np.isnan(wav.common_peak(p)) and wav.gain(wav.common_peak(p), normalise) == 1.0
    assert wav.common_peak(np.zeros(0, dtype=np.float32)) == 0
    with pytest.raises(wav.WavError, match="signals, channels, samples"):
        wav.encode_stems(stack[0], depth, normalise)


# ---- the Python surface, without a device -----------------------------------------------------------------------------------------------

CALLS = (d.render_piece, d.render_score, d.render_piece_pcm, d.render_score_pcm, d.render_piece_wav, d.render_score_wav)


def voices(n=3):
    d.configure(sv.SAMPLE_RATE)
    return [sv.voice(k) for k in range(n)]


@pytest.mark.parametrize("call", CALLS, ids=lambda f: f.__name__)
def test_stems_that_is_no_bool_is_refused_by_string_before_anything_else(call):
    for value in (1, 0, None, "mix", ["direct"], 2.0):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, stems=value, pans=[0])  # (the pans' shape would be refused next)
        assert str(e.value) == mix.STEMS_NOT_BOOL
    assert mix.check_stems(True) is True and mix.check_stems(np.bool_(False)) is False


def test_stems_travel_with_the_placement_to_the_piece():
    d.configure(sv.SAMPLE_RATE)
    assert render._placing(None, None, None, None, -3, None, False)["stems"] is False
    placing = render._placing(None, None, None, None, -3, None, False, None, [mc.echo], None, [mc.clip, None], [1, -1, 0], None, [[1, 0.5]], True)
    assert placing["stems"] is True
    *_, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, placing)
    assert place.stems is True and "stems" not in place.keywords() and place.tracks[0] == 2 and len(place.buses) == 1
    # a score with stems goes the piece's way, as one part
    with pytest.raises(descriptor.DuspError, match="the voices of a score are isomorphic circuits"):
        d.render_score([sv.voice(0), mc.stereo_voice(1)], [0, 1], 0.01, 0, stems=True)
    # a timeline of no samples renders nothing: every signal empty, by name
    with_tracks = dict(tracks=[mc.echo, None], track_of=[0, 1, -1], faders=[1, 0.5], buses=[mc.comb], track_sends=[[1, 0]])
    got = d.render_score(voices(), [0, 1, 2], 0.01, 0, stems=True, **with_tracks)
    assert isinstance(got, render.Stems) and got.names == ["direct", "track0", "track1", "bus0", "mix"] == mix.stem_names(2, 1)
    assert len(got.tracks) == 2 and len(got.buses) == 1 and len(got.mix) == 0 and got.mix.sampleRate == sv.SAMPLE_RATE and got["bus0"] is got.buses[0]
    assert set(got.peaks) == set(got.names) and got.peak == 0 and not hasattr(got, "gain")
    pcm = d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 2, stems=True)
    assert pcm.names == ["direct", "mix"] and pcm.tracks == [] and pcm.buses == [] and pcm.mix.data.shape == (0, 1, 3) and pcm.direct.bitDepth == 24 and pcm.gain == 1.0
    files = d.render_piece_wav(voices(), [0, 1, 2], 0.01, 0, 16, 0, stems=True, **with_tracks)
    assert files.names == got.names and all(f[:4] == b"RIFF" for f in [files.direct, files.mix] + files.tracks + files.buses)
    # without stems a call hands back what it did
    assert len(d.render_score(voices(), [0, 1, 2], 0.01, 0, stems=False, **with_tracks)) == 0


# ---- the kernels' text, under sanitizers ------------------------------------------------------------------------------------------------

def test_score_stems_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """the STEMS instances of the mix and return kernels (dusp_amd/csrc/score_tracks_engine.hip, score_send_engine.hip) and
    pcm_peak_common.hpp themselves, compiled for the host with their lanes run one after the other, every buffer a heap allocation of
    exactly its size, under AddressSanitizer and UBSan, against a brute-force loop and against the instances without stems
    (tests/native/score_stems_kernel_check.cpp lists what it covers).  A stand-alone program, run as a subprocess."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "score_stems_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub"), "-x", "c++",
                           os.path.join(native, "score_stems_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 3000 and rep["wide"] > 400 and rep["narrow"] > 2000 and rep["strided"] == 2 and rep["old"] > 3000, rep
