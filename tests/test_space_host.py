"""Space placement, on the CPU: dusp_amd.mix.score_chain_rows_placed — every voice heard by every speaker through a gain and a delay of
its own — over the oracle's renders of the voices IS the oracle's render of the anchor circuit, channel by channel, bit for bit
(tests/space_cases.py says what the anchor is and where it ends).  Then space_taps against the oracle's own Subtract -> VectorMagnitude
-> Multiply, the chain's algebra on planted rows, a brute-force loop per sample, the planner and the kernel's text on the host under
sanitizers, and the refusal strings of the Python and the JavaScript host, which need no device.  Bit patterns everywhere (for NaN, the
positions): no tolerances."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import score_voices as sv
from conftest import ROOT
from dusp_amd import descriptor, mix, runtime
from dusp_amd.mix import score_chain_rows, score_chain_rows_placed, space_taps
from space_cases import EDGE_DELAYS, RING, SDPM, SPEAKERS, anchor_circuit, decibels, layout, planted
from test_piece_host import NV_SAW, SANITIZE, bits, interleaved_voice, oracle_rows, same


def assert_bits(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0)))


# ---- the anchor: the oracle's one-channel circuits ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("n_speakers", [2, 3])
@pytest.mark.parametrize("n", [1, 2, 13, 37])
def test_the_placed_chain_over_the_voices_renders_is_the_anchor_circuit_channel_by_channel(n, n_speakers, with_gains, oracle):
    d.configure(sv.SAMPLE_RATE)
    onsets, gains, places, speakers, delays, tap_gains = layout(n, n_speakers)
    _, lengths, _ = sv.layout(n)  # (700 .. 773: beyond the Ramp's end, a length cuts off only zeros)
    g = gains if with_gains else None
    db = decibels(places, speakers)
    assert np.array_equal(tap_gains, np.vectorize(lambda x: math.pow(10, x / 20))(db)) and RING == 8192
    rows = [np.asarray(oracle.render(descriptor.extract(sv.voice(k)).words, sv.NV), dtype=np.float32) for k in range(n)]
    got = score_chain_rows_placed(rows, onsets, delays, tap_gains, sv.NT, gains=g)
    cut = score_chain_rows_placed(rows, onsets, delays, tap_gains, sv.NT, lengths=lengths, gains=g)
    rounded = score_chain_rows_placed(rows, onsets, np.round(delays), tap_gains, sv.NT, gains=g)
    assert got.shape == (n_speakers, sv.NT)
    for c in range(n_speakers):
        circuit = anchor_circuit([sv.voice(k) for k in range(n)], onsets, db, delays, c, g)
        want = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
        assert want.shape == (1, sv.NT) and np.abs(want).max() > 0
        assert_bits(got[c:c + 1], want)
        assert_bits(cut[c:c + 1], want)
        # the delays rounded to whole samples are another piece, wherever a voice with a fractional delay sounds
        if (delays[:, c] != np.floor(delays[:, c])).any():
            assert (bits(rounded[c]) != bits(want[0])).sum() >= 200


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("n", [2, 13])
def test_the_placed_chain_over_the_parts_renders_is_the_interleaved_piece(n, with_gains, oracle):
    rows = oracle_rows(n, oracle)  # (773 and 1031 samples in turn, rendered part by part)
    assert [r.shape for r in rows] == [(1, sv.NV if k % 2 == 0 else NV_SAW) for k in range(n)]
    onsets, gains, places, speakers, delays, tap_gains = layout(n, 2)
    g = gains if with_gains else None
    db = decibels(places, speakers)
    d.configure(sv.SAMPLE_RATE)
    got = score_chain_rows_placed(rows, onsets, delays, tap_gains, sv.NT, gains=g)
    for c in range(2):
        circuit = anchor_circuit([interleaved_voice(k) for k in range(n)], onsets, db, delays, c, g)
        assert_bits(got[c:c + 1], np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32))


def test_space_taps_is_the_oracles_subtract_magnitude_multiply(oracle):
    """20 random places in three dimensions against three speakers: dist * dBpm and dist * sdpm as the reference's units compute them,
    read past the first chunk (a unit whose inlet comes from another ticks a chunk late)"""
    d.configure(sv.SAMPLE_RATE)
    rs = np.random.RandomState(11)
    places = rs.uniform(-40, 40, (20, 3))
    places[0] = [0.5, -0.25, 3.0]
    speakers = [[0.5, -0.25, 3.0], [-1.0, 0.0, 0.0], [7.125, 1e-3, -2.0]]
    dbpm, sdpm = -3.0, sv.SAMPLE_RATE / 343
    delays, gains = space_taps(places, speakers, sample_rate=sv.SAMPLE_RATE)
    assert delays.shape == gains.shape == (20, 3) and delays[0, 0] == 0 and gains[0, 0] == 1
    again = space_taps(places, speakers, dbpm, sdpm)
    assert np.array_equal(again[0], delays) and np.array_equal(again[1], gains) and d.space_taps is space_taps
    for k in range(20):
        for c in range(3):
            def scaled(factor):
                sub = d.Subtract([float(x) for x in places[k]], [float(x) for x in speakers[c]])
                mag = d.VectorMagnitude()
                mag.IN = sub
                return np.asarray(oracle.render(descriptor.extract(d.Multiply(mag, factor)).words, 1024), dtype=np.float32)[0, 1000]
            db = scaled(dbpm)
            assert np.float32(delays[k, c]).view(np.uint32) == scaled(sdpm).view(np.uint32) and delays[k, c] == np.float64(np.float32(delays[k, c])), (k, c)
            assert gains[k, c] == math.pow(10, float(db) / 20), (k, c)
    # one and two coordinates; the default speakers are the reference's stereo pair
    one = space_taps([[2.0], [-1.0]], [[0.0]], sample_delay_per_metre=100)
    assert one[0].tolist() == [[200.0], [100.0]] and one[1][0, 0] == math.pow(10, float(np.float32(2.0) * np.float32(-3)) / 20)
    assert np.array_equal(space_taps([[0, 1]], sample_delay_per_metre=10)[0], space_taps([[0, 1]], [[-1, 0], [1, 0]], sample_delay_per_metre=10)[0])


# ---- the chain's algebra on planted rows ------------------------------------------------------------------------------------------------

N_PLANTED = 13


def test_the_planted_cases_hold_what_they_are_built_to_hold():
    rows, onsets, lengths, gains, delays, tap_gains, init = planted(37, 3)
    assert set(delays.ravel().tolist()) == set(EDGE_DELAYS) | {2000.0} and delays[2, 1] == 2000.0 and init.shape == (3, 1301)
    assert {r.shape[1] for r in rows} == {773, 1, 255, 0, 257, 3} and (onsets < 0).any() and (lengths == 0).any()
    flat = np.concatenate([r.reshape(-1) for r in rows])
    assert np.isnan(flat).any() and np.isinf(flat).any() and (np.signbit(flat) & (flat == 0)).any() and ((flat != 0) & (np.abs(flat) < np.finfo(np.float32).tiny)).any()
    raw = score_chain_rows_placed(rows, onsets, delays, tap_gains, 1301, lengths=lengths, raw=True)
    assert np.isnan(raw).any() and not np.isnan(score_chain_rows_placed(rows, onsets, delays, tap_gains, 1301, lengths=lengths)).any()
    whole = score_chain_rows_placed(rows, onsets, np.floor(delays), tap_gains, 1301, lengths=lengths, raw=True)
    assert (bits(raw) != bits(whole)).mean() > 0.2  # (the fractions are heard)


@pytest.mark.parametrize("n_speakers", [1, 2, 3, 6])
def test_every_delay_zero_and_every_gain_one_is_the_mono_chain_on_each_channel(n_speakers):
    rows, onsets, lengths, gains, _, _, init = planted(N_PLANTED, n_speakers)
    zeros, ones = np.zeros((N_PLANTED, n_speakers)), np.ones((N_PLANTED, n_speakers))
    for kw in ({}, {"lengths": lengths, "gains": gains}, {"gains": gains}):
        for raw in (True, False):
            for with_init in (False, True):
                got = score_chain_rows_placed(rows, onsets, zeros, ones, 1301, raw=raw, init=init if with_init else None, **kw)
                for c in range(n_speakers):
                    want = score_chain_rows(rows, onsets, 1301, raw=raw, init=init[c:c + 1] if with_init else None, **kw)
                    assert same(got[c:c + 1], want), (sorted(kw), raw, with_init, c)
    # a whole delay is the voice shifted: the mono chain with onset + delay
    shifts = np.arange(N_PLANTED) * 7 % 300
    got = score_chain_rows_placed(rows, onsets, np.repeat(shifts[:, None], n_speakers, axis=1).astype(np.float64), ones, 1301, lengths=lengths, gains=gains, raw=True)
    want = score_chain_rows(rows, onsets + shifts, 1301, lengths=lengths, gains=gains, raw=True)
    assert all(same(got[c:c + 1], want) for c in range(n_speakers))


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("n_speakers", [2, 3])
def test_a_placed_chain_cut_at_every_voice_and_continued_is_the_same_chain(n_speakers, with_gains):
    rows, onsets, lengths, gains, delays, tap_gains, _ = planted(N_PLANTED, n_speakers)
    n, n_total = len(rows), 1301
    g = gains if with_gains else None
    cut_of = lambda a, lo, hi: None if a is None else a[lo:hi]
    chain = lambda lo, hi, **kw: score_chain_rows_placed(rows[lo:hi], onsets[lo:hi], delays[lo:hi], tap_gains[lo:hi], n_total, lengths=lengths[lo:hi], gains=cut_of(g, lo, hi), **kw)
    whole_raw, whole = chain(0, n, raw=True), chain(0, n)
    for cut in range(0, n + 1):
        head = chain(0, cut, raw=True) if cut else np.zeros(whole.shape, dtype=np.float32)
        for raw, want in ((True, whole_raw), (False, whole)):
            assert same(chain(cut, n, init=head, raw=raw), want), (cut, raw)
    # a -0 partial sum survives voices that do not cover the sample on THAT channel, and leaves as +0
    init = np.full(whole.shape, -0.0, dtype=np.float32)
    cont = chain(0, n, init=init, raw=True)
    for c in range(n_speakers):
        uncovered = np.ones(n_total, dtype=bool)
        for k in range(n):
            if lengths[k] > 0:
                at = int(onsets[k]) + int(np.floor(delays[k, c]))
                uncovered[max(at, 0):max(at + int(lengths[k]) + (1 if delays[k, c] != np.floor(delays[k, c]) else 0), 0)] = False
        assert uncovered.any() and np.signbit(cont[c, uncovered]).all() and (cont[c, uncovered] == 0).all()
        assert not np.signbit(chain(0, n, init=init)[c, uncovered]).any()


@pytest.mark.parametrize("n_speakers", [2, 3])
def test_the_timeline_cut_into_windows_is_the_whole(n_speakers):
    """window edges on, one before and one after every edge of every voice's span on every channel"""
    rows, onsets, lengths, gains, delays, tap_gains, _ = planted(N_PLANTED, n_speakers)
    edges = set()
    for k in range(N_PLANTED):
        for c in range(n_speakers):
            at = int(onsets[k]) + int(np.floor(delays[k, c]))
            end = at + int(lengths[k]) + (1 if delays[k, c] != np.floor(delays[k, c]) else 0)
            edges |= {at + e for e in (-1, 0, 1)} | {end + e for e in (-1, 0, 1)}
    cuts = sorted(c for c in edges | {1, 256, 1300} if 0 < c < 1301)
    assert len(cuts) > 40
    for raw in (True, False):
        whole = score_chain_rows_placed(rows, onsets, delays, tap_gains, 1301, lengths=lengths, gains=gains, raw=raw)
        for cut in cuts:
            first = score_chain_rows_placed(rows, onsets, delays, tap_gains, cut, lengths=lengths, gains=gains, raw=raw)
            second = score_chain_rows_placed(rows, onsets - cut, delays, tap_gains, 1301 - cut, lengths=lengths, gains=gains, raw=raw)  # (onsets shifted: many are negative now)
            assert same(np.concatenate([first, second], axis=1), whole), (raw, cut)


# ---- a brute-force loop per sample --------------------------------------------------------------------------------------------------------

def brute(rows, onsets, delays, tap_gains, n_total, lengths, gains=None):
    """the contract as the issue writes it, one channel, one timeline sample and one voice at a time, in numpy scalars"""
    f32, f64 = np.float32, np.float64
    n_ch = np.asarray(delays).shape[1]
    out = np.zeros((n_ch, n_total), dtype=f32)
    with np.errstate(all="ignore"):
        for c in range(n_ch):
            for t in range(n_total):
                acc = f32(0)
                for k, row in enumerate(rows):
                    D, G = f64(delays[k][c]), f64(tap_gains[k][c])
                    i = math.floor(D)
                    w1 = D - f64(i)
                    w0 = f64(1.0) - w1
                    length, s = int(lengths[k]), t - int(onsets[k]) - i

                    def y(at):
                        v = row[0, at]
                        if gains is not None:
                            v = f32(v * f32(gains[k]))
                        return f32(G * f64(v))
                    if w1 == 0:
                        if 0 <= s < length:
                            acc = f32(acc + y(s))
                        continue
                    if length == 0 or s < 0 or s > length:
                        continue
                    if s == 0:
                        term = f32(f64(y(0)) * w0)
                    else:
                        ceil_tap = f32(f64(y(s - 1)) * w1)
                        term = ceil_tap if s == length else f32(f64(ceil_tap) + f64(y(s)) * w0)
                    acc = f32(acc + term)
                out[c, t] = acc
    return out


def test_edge_voices_against_a_loop_per_sample():
    rng = np.random.RandomState(78)
    n_total = 40
    for length, onset in [(1, 5), (1, -1), (1, n_total - 1), (7, -1), (7, -7), (7, -8), (7, n_total - 7), (7, n_total - 8), (7, n_total), (7, 0), (0, 3), (45, -2), (7, -20)]:
        for taps in ([0.0, 0.5], [2.0 ** -24, 3.0], [1.0 - 2.0 ** -53, 12.25], [41.0, 40.5], [14.0, 13.5]):
            samples = max(length, 1) + 2  # (the row is longer than the length: what lies behind it is not heard)
            row = (rng.standard_normal((1, samples)) * 3).astype(np.float32)
            if samples > 3:
                row[0, 1], row[0, 2] = -0.0, np.inf
            other = rng.standard_normal((1, 9)).astype(np.float32)  # a second voice under it
            rows, onsets, lengths, gains = [other, row], [11, onset], [9, length], np.array([0.7, -1.3], dtype=np.float32)
            delays, tap_gains = [[0.0, 2.5], taps], [[1.0, 0.5], [math.pow(10, -4.5 / 20), -2.0]]
            for g in (None, gains):
                got = score_chain_rows_placed(rows, onsets, delays, tap_gains, n_total, lengths=lengths, gains=g, raw=True)
                assert same(got, brute(rows, onsets, delays, tap_gains, n_total, lengths, g)), (length, onset, taps, g is not None)
    x = np.array([[1.0, 2.0, 4.0]], dtype=np.float32)
    assert score_chain_rows_placed([x], [-3], [[0.25, 3.0]], [[1.0, 0.5]], 4).tolist() == [[1.0, 0, 0, 0], [0.5, 1.0, 2.0, 0]]
    assert score_chain_rows_placed([x], [0], [[1.25]], [[2.0]], 4).tolist() == [[0, 1.5, 3.5, 7.0]]
    # onsets at the int64 limits: the shifted span leaves int64 and takes no part; nothing wraps
    far = score_chain_rows_placed([x, x], [2 ** 63 - 1, -2 ** 63], [[5.5, 0.0], [2.0 ** 24, 0.5]], [[1.0, 1.0], [1.0, 1.0]], 8)
    assert far.shape == (2, 8) and not far.any()


# ---- the planner and the kernel's text, under sanitizers ----------------------------------------------------------------------------------

def test_score_rows_plan_with_taps_against_brute_force_under_sanitizers(tmp_path):
    """score_rows_plan of dusp_amd/csrc/score_plan.hpp with taps (tests/native/score_rows_plan_space_check.cpp lists what it covers)"""
    exe = str(tmp_path / "score_rows_plan_space_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + SANITIZE + [os.path.join(ROOT, "tests", "native", "score_rows_plan_space_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 6000 and rep["doubled"] >= 100 and rep["far_onsets"] >= 1000 and rep["disjoint"] >= 1000, rep
    assert rep["two_taps"] >= 10000 and rep["zero_taps"] >= 100, rep


def test_score_space_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/score_space_engine.hip itself, compiled for the host with its lanes run one after the other, every row and the tap
    array a heap allocation of exactly its size, under AddressSanitizer and UBSan: a read of row[len] or row[-1] is caught here
    (tests/native/score_space_kernel_check.cpp lists what it covers)."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "score_space_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub"), "-x", "c++",
                           os.path.join(native, "score_space_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 3000 and rep["doubled"] >= 100 and rep["windows"] >= 50, rep
    assert rep["two_taps"] > 1000000 and rep["one_taps"] > 1000000 and rep["outside"] >= 1000 and rep["whole_lists"] >= 100, rep


# ---- argument checks and refusal strings, Python and JavaScript, without a device ---------------------------------------------------------

SHAPE = "dusp-hip: places must have shape (voices=3, 1 .. 3 coordinates)"
FINITE = "dusp-hip: the place of voice 2 is not finite"
SPEAKER_FINITE = "dusp-hip: the place of speaker 1 is not finite"
COORDINATES = "dusp-hip: places have 2 coordinates, speakers have 3: the same number"
SPEAKER_COUNT = "dusp-hip: a Space has 1 .. 8 speakers, not 9"
ALONE = "dusp-hip: places stand alone: together with pans or fracs they are refused (a sub-sample onset in front of a Space would be a second two-tap stage)"
MONO = "dusp-hip: a placed voice is mono: part 0 has 2 output channels"
ONE_PART = "dusp-hip: the voices of a score are isomorphic circuits: a piece renders several instruments"
TOO_FAR = "dusp-hip: the delay of voice 1 at speaker 0 is outside [0, 2^24] samples"


def python_refusals():
    import mix_voices
    d.configure(sv.SAMPLE_RATE)
    mono = lambda: [sv.voice(0), sv.voice(1), sv.voice(2)]
    two = lambda: [sv.voice(0), mix_voices.voice("filtered_saw", 0), sv.voice(1)]
    stereo = lambda: [mix_voices.voice("pan", k) for k in range(3)]
    at = [[0, 0], [1, 1], [2, 0.5]]
    calls = {
        "shape": lambda: d.render_piece(mono(), [0, 1, 2], 0.01, 0.05, places=[[0, 0], [1, 1]]),
        "shapeScore": lambda: d.render_score(mono(), [0, 1, 2], 0.01, 0.05, places=[[0, 0, 0, 0]] * 3),
        "finite": lambda: d.render_piece(mono(), [0, 1, 2], 0.01, 0.05, places=[[0, 0], [1, 1], [float("nan"), 0]]),
        "finitePcm": lambda: d.render_score_pcm(mono(), [0, 1, 2], 0.01, 0.05, places=[[0, 0], [1, 1], [0, float("inf")]]),
        "finiteWav": lambda: d.render_piece_wav(mono(), [0, 1, 2], 0.01, 0.05, places=[[0, 0], [1, 1], [0, float("-inf")]]),
        "speakerFinite": lambda: d.render_piece(mono(), [0, 1, 2], 0.01, 0.05, places=at, speakers=[[0, 0], [float("nan"), 1]]),
        "coordinates": lambda: d.render_piece_pcm(mono(), [0, 1, 2], 0.01, 0.05, places=at, speakers=[[0, 0, 0]]),
        "speakerCount": lambda: d.render_score_wav(mono(), [0, 1, 2], 0.01, 0.05, places=at, speakers=[[0, k] for k in range(9)]),
        "pans": lambda: d.render_piece(mono(), [0, 1, 2], 0.01, 0.05, places=at, pans=[0, 0, 0]),
        "fracs": lambda: d.render_score(mono(), [0, 1, 2], 0.01, 0.05, places=at, fracs=[0, 0, 0]),
        "mono": lambda: d.render_piece(stereo(), [0, 1, 2], 0.01, 0.05, places=at),
        "onePart": lambda: d.render_score(two(), [0, 1, 2], 0.01, 0.05, places=at),
        "tooFar": lambda: d.render_piece(mono(), [0, 1, 2], 0.01, 0.05, places=[[0, 0], [3e5, 0], [0, 0]], speakers=[[0, 0]]),
    }
    got = {}
    for name, call in calls.items():
        with pytest.raises((ValueError, descriptor.DuspError)) as e:
            call()
        got[name] = str(e.value)
    return got


def test_python_refuses_by_string_before_anything_is_built():
    r = python_refusals()
    assert r["shape"] == r["shapeScore"] == SHAPE and r["finite"] == r["finitePcm"] == r["finiteWav"] == FINITE and r["speakerFinite"] == SPEAKER_FINITE
    assert r["coordinates"] == COORDINATES and r["speakerCount"] == SPEAKER_COUNT and r["pans"] == r["fracs"] == ALONE and r["mono"] == MONO
    assert r["onePart"] == ONE_PART and r["tooFar"] == TOO_FAR
    a, b = np.zeros((1, 5), np.float32), np.zeros((1, 3), np.float32)
    ok = [[0.0, 1.5], [2.0, 0.0]]
    for delays, gains, message in ((ok[:1], ok[:1], "dusp-hip: the taps' delays and gains must both have shape (voices=2, speakers)"),
                                   (ok, [[1.0], [1.0]], "dusp-hip: the taps' delays and gains must both have shape (voices=2, speakers)"),
                                   ([[0.0] * 9] * 2, [[1.0] * 9] * 2, "dusp-hip: a Space has 1 .. 8 speakers, not 9"),
                                   ([[0.0, np.nan], [0, 0]], ok, "dusp-hip: the delay of voice 0 at speaker 1 is not finite"),
                                   ([[0.0, 0.0], [-2.0 ** -60, 0]], ok, "dusp-hip: the delay of voice 1 at speaker 0 is outside [0, 2^24] samples"),
                                   ([[0.0, 0.0], [0, 2.0 ** 24 + 2]], ok, "dusp-hip: the delay of voice 1 at speaker 1 is outside [0, 2^24] samples"),
                                   (ok, [[1.0, 1.0], [np.inf, 1.0]], "dusp-hip: the gain of voice 1 at speaker 0 is not finite")):
        for call in (lambda: score_chain_rows_placed([a, b], [0, 1], delays, gains, 9), lambda: runtime.tap_arrays((delays, gains), 2)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == message
    with pytest.raises(ValueError, match="every placed row must be mono"):
        score_chain_rows_placed([np.zeros((2, 5), np.float32)], [0], [[0.0]], [[1.0]], 9)
    with pytest.raises(ValueError, match="onsets are whole numbers"):
        score_chain_rows_placed([a, b], [0, 0.5], ok, ok, 9)
    assert score_chain_rows_placed([a, b], [0, 1], [[0.0, 2.0 ** 24], [1.0 - 2.0 ** -53, 5]], ok, 9).shape == (2, 9)
    dl, tg = runtime.tap_arrays(([[0, 1.5]], [[np.float32(0.5), 1]]), 1)
    assert dl.dtype == tg.dtype == np.float64 and dl.flags.c_contiguous and dl.tolist() == [[0, 1.5]] and tg.tolist() == [[0.5, 1]]
    with pytest.raises(ValueError, match="voice_duration is one number"):
        d.render_score([sv.voice(0), sv.voice(1)], [0, 1], [0.01, 0.01], 0.05, places=[[0, 0], [1, 1]])
    # a timeline of no samples: nothing to render, checked all the same
    assert len(d.render_piece([sv.voice(0), sv.voice(1)], [0, 1], 0.01, 0, places=[[0, 0], [1, 1]])) == 0
    assert d.render_piece_pcm([sv.voice(0), sv.voice(1)], [0, 1], 0.01, 0, places=[[0, 0], [1, 1]], speakers=SPEAKERS[3]).data.shape == (0, 3)
    # the symbols a binder looks for
    L = runtime.load()
    assert hasattr(L, "dusp_score_rows_space_device") and hasattr(L, "dusp_render_host_score_parts_space")
    assert "dusp_score_rows_space_device" in runtime.EXPORTS and "dusp_render_host_score_parts_space" in runtime.EXPORTS


def test_the_javascript_host_refuses_with_pythons_strings():
    node = shutil.which("node")
    assert node is not None, "node is needed for the JavaScript host"
    addon = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")
    if not os.path.exists(addon):
        subprocess.check_call(["make", "-C", os.path.dirname(addon), "-s"])
    p = subprocess.run([node, os.path.join(ROOT, "tests", "js", "check_space.js"), "--sampleRate=48000", "refusals"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    assert rep["refusals"] == python_refusals(), rep["refusals"]
    assert rep["addonCall"] is True
    # spaceTaps is space_taps: the delays bit for bit, the gains by each host's own pow (equal here)
    places = [[0, 0], [1, 2], [-2.5, 0.75], [1, 0]]
    delays, gains = space_taps(places, sample_rate=48000)
    assert rep["taps"]["delays"] == delays.ravel().tolist() and rep["taps"]["gains"] == gains.ravel().tolist() and rep["taps"]["nSpeakers"] == 2
    three = space_taps([[0, 0, 1], [3, -1, 2]], SPEAKERS_3D, -6, 77.5)
    assert rep["taps3"]["delays"] == three[0].ravel().tolist() and rep["taps3"]["gains"] == three[1].ravel().tolist()


SPEAKERS_3D = [[-1, 0, 0], [1, 0, 0], [0, 2, 1]]
