"""Sub-sample onsets, on the CPU: dusp_amd.mix.score_chain_rows / score_chain_rows_panned with `fracs` — a voice at onset + fraction
samples is heard through the reference Delay's two taps — over the oracle's renders of the voices IS the oracle's render of
`Sum.many(Delay(Pan(Multiply(voice_k, g_k), pan_k), onset_k + frac_k, ring))` as one circuit, bit for bit (tests/frac_cases.py says
where that anchor ends).  Then the chain's algebra on planted rows, edge voices against a brute-force loop per sample, split_onsets,
the planner and the kernel's text on the host under sanitizers, and the refusal strings of the Python and the JavaScript host, which
need no device.  Bit patterns everywhere (for NaN, the positions): no tolerances."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import score_voices as sv
from conftest import ROOT
from dusp_amd import descriptor, mix, runtime
from dusp_amd.mix import score_chain_rows, score_chain_rows_panned, split_onsets, two_tap_terms
from frac_cases import EDGE_FRACS, RING, as_one_frac_circuit, layout, pans_for, planted, planted_wide
from test_piece_host import NV_SAW, SANITIZE, bits, interleaved_voice, oracle_rows, same


def assert_bits(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0)))


def chain(rows, onsets, pans, n_total, **kw):
    """the mono chain, or with pans the panned one"""
    return score_chain_rows(rows, onsets, n_total, **kw) if pans is None else score_chain_rows_panned(rows, onsets, pans, n_total, **kw)


# ---- the anchor: the oracle's one circuit -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("n,panned", [(1, False), (2, False), (13, False), (37, False), (2, True), (13, True), (37, True)])
def test_the_two_tap_chain_over_the_voices_renders_is_sum_many_of_fractional_delays(n, panned, with_gains, oracle):
    d.configure(sv.SAMPLE_RATE)
    onsets, fracs, gains = layout(n, panned)
    _, lengths, _ = sv.layout(n)  # (700 .. 773: beyond the Ramp's end, a length cuts off only zeros)
    g = gains if with_gains else None
    pans = pans_for(n) if panned else None
    assert (fracs != 0).any() and (n < 4 or ((fracs == 0).any() and (fracs == 0.5).any() and (fracs == 1 / 1024).any())) and RING == 8192
    rows = [np.asarray(oracle.render(descriptor.extract(sv.voice(k)).words, sv.NV), dtype=np.float32) for k in range(n)]
    circuit = as_one_frac_circuit([sv.voice(k) for k in range(n)], onsets, fracs, g, pans)
    want = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
    assert want.shape == (2 if panned else 1, sv.NT) and np.abs(want).max() > 0
    assert_bits(chain(rows, onsets, pans, sv.NT, lengths=lengths, gains=g, fracs=fracs), want)
    assert_bits(chain(rows, onsets, pans, sv.NT, gains=g, fracs=fracs), want)
    # rounding the onsets to whole samples is another piece: a voice with a fraction sounds for 700 samples, and nearly all of them differ
    assert (bits(chain(rows, onsets, pans, sv.NT, lengths=lengths, gains=g)) != bits(want)).sum() >= 600


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("panned", [False, True], ids=["mono", "panned"])
@pytest.mark.parametrize("n", [2, 13, 37])
def test_the_two_tap_chain_over_the_parts_renders_is_the_interleaved_piece(n, panned, with_gains, oracle):
    rows = oracle_rows(n, oracle)  # (773 and 1031 samples in turn, rendered part by part)
    assert [r.shape for r in rows] == [(1, sv.NV if k % 2 == 0 else NV_SAW) for k in range(n)]
    onsets, fracs, gains = layout(n, panned)
    g = gains if with_gains else None
    pans = pans_for(n) if panned else None
    d.configure(sv.SAMPLE_RATE)
    circuit = as_one_frac_circuit([interleaved_voice(k) for k in range(n)], onsets, fracs, g, pans)
    want = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
    assert_bits(chain(rows, onsets, pans, sv.NT, gains=g, fracs=fracs), want)


# ---- the chain's algebra on planted rows ------------------------------------------------------------------------------------------------

N_PLANTED = 13
KINDS = ["mono", "wide", "panned"]


def planted_case(kind):
    rows, onsets, lengths, gains, pans, init, fracs = planted_wide(N_PLANTED) if kind == "wide" else planted(N_PLANTED)
    return rows, onsets, lengths, gains, pans if kind == "panned" else None, init[:len(rows[0])] if kind != "panned" else init, fracs


def test_the_planted_cases_hold_what_they_are_built_to_hold():
    rows, onsets, lengths, gains, pans, init, fracs = planted(37)
    assert set(fracs.tolist()) == set(EDGE_FRACS) and {0.0, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -53} <= set(EDGE_FRACS) and 1.0 - (1.0 - 2.0 ** -53) == 2.0 ** -53
    assert {r.shape[1] for r in rows} == {773, 1, 255, 0, 257, 3} and (onsets < 0).any() and (lengths == 0).any()
    flat = np.concatenate([r.reshape(-1) for r in rows])
    assert np.isnan(flat).any() and np.isinf(flat).any() and (np.signbit(flat) & (flat == 0)).any() and ((flat != 0) & (np.abs(flat) < np.finfo(np.float32).tiny)).any()
    assert all(r.shape[0] == 2 for r in planted_wide(37)[0])
    for kind in KINDS:
        rows, onsets, lengths, gains, pans, _, fracs = planted_case(kind)
        raw = chain(rows, onsets, pans, 1301, lengths=lengths, fracs=fracs, raw=True)
        assert np.isnan(raw).any() and not np.isnan(chain(rows, onsets, pans, 1301, lengths=lengths, fracs=fracs)).any()
        assert (bits(raw) != bits(chain(rows, onsets, pans, 1301, lengths=lengths, raw=True))).mean() > 0.3, kind  # (the fractions are heard)


@pytest.mark.parametrize("kind", KINDS)
def test_all_fractions_zero_is_the_chain_without_fractions(kind):
    rows, onsets, lengths, gains, pans, init, _ = planted_case(kind)
    zeros = np.zeros(len(rows))
    for kw in ({}, {"lengths": lengths, "gains": gains}, {"lengths": lengths, "init": init}, {"gains": gains, "init": init}):
        for raw in (True, False):
            assert same(chain(rows, onsets, pans, 1301, fracs=zeros, raw=raw, **kw), chain(rows, onsets, pans, 1301, raw=raw, **kw)), (sorted(kw), raw)
            assert same(chain(rows, onsets, pans, 1301, fracs=None, raw=raw, **kw), chain(rows, onsets, pans, 1301, raw=raw, **kw))


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_two_tap_chain_cut_at_every_voice_and_continued_is_the_same_chain(kind, with_gains):
    rows, onsets, lengths, gains, pans, _, fracs = planted_case(kind)
    n, n_total = len(rows), 1301
    g = gains if with_gains else None
    cut_of = lambda a, lo, hi: None if a is None else a[lo:hi]
    whole_raw, whole = chain(rows, onsets, pans, n_total, lengths=lengths, gains=g, fracs=fracs, raw=True), chain(rows, onsets, pans, n_total, lengths=lengths, gains=g, fracs=fracs)
    for cut in range(0, n + 1):
        head = (chain(rows[:cut], onsets[:cut], cut_of(pans, 0, cut), n_total, lengths=lengths[:cut], gains=cut_of(g, 0, cut), fracs=fracs[:cut], raw=True) if cut
                else np.zeros(whole.shape, dtype=np.float32))
        for raw, want in ((True, whole_raw), (False, whole)):
            got = chain(rows[cut:], onsets[cut:], cut_of(pans, cut, n), n_total, lengths=lengths[cut:], gains=cut_of(g, cut, n), fracs=fracs[cut:], init=head, raw=raw)
            assert same(got, want), (cut, raw)
    # a -0 partial sum survives voices that do not cover the sample — the tail tap's sample IS covered — and leaves as +0
    uncovered = np.ones(n_total, dtype=bool)
    for k in range(n):
        uncovered[max(int(onsets[k]), 0):max(int(onsets[k] + lengths[k]) + (1 if fracs[k] != 0 and lengths[k] > 0 else 0), 0)] = False
    assert uncovered.any()
    init = np.full(whole.shape, -0.0, dtype=np.float32)
    cont = chain(rows, onsets, pans, n_total, lengths=lengths, gains=g, fracs=fracs, init=init, raw=True)
    assert np.signbit(cont[:, uncovered]).all() and (cont[:, uncovered] == 0).all()
    assert not np.signbit(chain(rows, onsets, pans, n_total, lengths=lengths, gains=g, fracs=fracs, init=init)[:, uncovered]).any()


@pytest.mark.parametrize("kind", KINDS)
def test_the_timeline_cut_into_windows_is_the_whole(kind):
    """window edges on, one before and one after every voice's tail sample (onset + len), and on its first"""
    rows, onsets, lengths, gains, pans, _, fracs = planted_case(kind)
    tails = sorted({int(t) + e for t in (onsets + lengths) for e in (-1, 0, 1)} | {int(o) + e for o in onsets for e in (0, 1)} | {1, 256, 1300})
    cuts = [c for c in tails if 0 < c < 1301]
    assert len(cuts) > 30
    for raw in (True, False):
        whole = chain(rows, onsets, pans, 1301, lengths=lengths, gains=gains, fracs=fracs, raw=raw)
        for cut in cuts:
            first = chain(rows, onsets, pans, cut, lengths=lengths, gains=gains, fracs=fracs, raw=raw)
            second = chain(rows, onsets - cut, pans, 1301 - cut, lengths=lengths, gains=gains, fracs=fracs, raw=raw)  # (onsets shifted: many are negative now)
            assert same(np.concatenate([first, second], axis=1), whole), (raw, cut)


# ---- edge voices against a brute-force loop per sample ----------------------------------------------------------------------------------

def brute(rows, onsets, fracs, n_total, lengths, gains=None, pans=None):
    """the contract as the issue writes it, one timeline sample and one voice at a time, in numpy scalars"""
    f32, f64 = np.float32, np.float64
    n_ch = 2 if pans is not None else rows[0].shape[0]
    out = np.zeros((n_ch, n_total), dtype=f32)
    with np.errstate(all="ignore"):
        for c in range(n_ch):
            for t in range(n_total):
                acc = f32(0)
                for k, row in enumerate(rows):
                    length, s = int(lengths[k]), t - int(onsets[k])

                    def x(at):
                        v = row[0 if pans is not None else c, at]
                        if gains is not None:
                            v = f32(v * f32(gains[k]))
                        if pans is not None:
                            side = f64(1) - f64(f32(pans[k])) if c == 0 else f64(1) + f64(f32(pans[k]))
                            v = f32(((f64(v) * side) / f64(2)) * mix.pan_comp([pans[k]])[0])
                        return v
                    if fracs[k] == 0:
                        if 0 <= s < length:
                            acc = f32(acc + x(s))
                        continue
                    if length == 0 or s < 0 or s > length:
                        continue
                    w1 = f64(fracs[k])
                    w0 = f64(1.0) - w1
                    if s == 0:
                        term = f32(f64(x(0)) * w0)
                    else:
                        ceil_tap = f32(f64(x(s - 1)) * w1)
                        term = ceil_tap if s == length else f32(f64(ceil_tap) + f64(x(s)) * w0)
                    acc = f32(acc + term)
                out[c, t] = acc
    return out


@pytest.mark.parametrize("panned", [False, True], ids=["plain", "panned"])
def test_edge_voices_against_a_loop_per_sample(panned):
    rng = np.random.RandomState(77)
    n_total = 40
    for length, onset in [(1, 5), (1, -1), (1, n_total - 1), (7, -1), (7, -7), (7, -8), (7, -6), (7, n_total - 7), (7, n_total - 8), (7, n_total - 1), (7, n_total), (7, 0),
                          (0, 3), (45, -2)]:
        for frac in (0.5, 2.0 ** -24, 1.0 - 2.0 ** -53, 0.3, 0.0):
            samples = max(length, 1) + 2  # (the row is longer than the length: what lies behind it is not heard)
            row = (rng.standard_normal((1 if panned else 2, samples)) * 3).astype(np.float32)
            if samples > 3:
                row[0, 1], row[0, 2] = -0.0, np.inf
            other = (rng.standard_normal((1 if panned else 2, 9))).astype(np.float32)  # a second voice under it, whole
            rows, onsets, fracs, lengths, gains = [other, row], [11, onset], [0.0, frac], [9, length], np.array([0.7, -1.3], dtype=np.float32)
            pans = np.array([0.3, -0.6], dtype=np.float32) if panned else None
            for g in (None, gains):
                got = chain(rows, onsets, pans, n_total, lengths=lengths, gains=g, fracs=fracs, raw=True)
                assert same(got, brute(rows, onsets, fracs, n_total, lengths, g, pans)), (length, onset, frac, g is not None)
    # the tail tap alone (onset = -len), and clipped off (onset + len = n_total)
    x = np.array([[1.0, 2.0, 4.0]], dtype=np.float32)
    assert score_chain_rows([x], [-3], 4, fracs=[0.25]).tolist() == [[1.0, 0, 0, 0]] and score_chain_rows([x], [-3], 4).tolist() == [[0, 0, 0, 0]]
    assert score_chain_rows([x], [1], 4, fracs=[0.25]).tolist() == [[0, 0.75, 1.75, 3.5]] and score_chain_rows([x], [-4], 4, fracs=[0.25]).tolist() == [[0, 0, 0, 0]]
    assert two_tap_terms(x, 0.25).tolist() == [[0.75, 1.75, 3.5, 1.0]]


def test_the_ceil_tap_is_rounded_to_f32_before_the_floor_tap_is_added():
    """c(s) = f32(f64(x[s-1]) * w1) alone in its slot: not the f64 product carried into the sum"""
    x = np.array([[1.0 + 2.0 ** -23, 1.0]], dtype=np.float32)
    frac = 1.0 / 3
    got = two_tap_terms(x, frac)[0, 1]
    c = np.float32(np.float64(x[0, 0]) * np.float64(frac))
    assert got == np.float32(np.float64(c) + np.float64(x[0, 1]) * (np.float64(1.0) - np.float64(frac)))
    xs = (np.random.RandomState(5).standard_normal((1, 4000))).astype(np.float32)
    carried = (xs[0, :-1].astype(np.float64) * frac + xs[0, 1:].astype(np.float64) * (1.0 - frac)).astype(np.float32)
    assert (bits(two_tap_terms(xs, frac)[0, 1:-1]) != bits(carried)).any()


# ---- split_onsets -----------------------------------------------------------------------------------------------------------------------

def test_split_onsets_floors_positions_of_any_sign():
    on, fr = split_onsets([0, 5, -5, 5538.46153846, -0.25, -3.75, 1 / 3, 2.0 ** 53, -2.0 ** 53, 2.0 ** 53 - 1, 2.0 ** 51 + 0.5, -(2.0 ** 62), 2.0 ** 62, np.nextafter(1.0, 0)])
    assert on.dtype == np.int64 and fr.dtype == np.float64
    assert on.tolist() == [0, 5, -5, 5538, -1, -4, 0, 2 ** 53, -2 ** 53, 2 ** 53 - 1, 2 ** 51, -2 ** 62, 2 ** 62, 0]
    assert fr.tolist() == [0, 0, 0, 5538.46153846 - 5538, 0.75, 0.25, 1 / 3, 0, 0, 0, 0.5, 0, 0, np.nextafter(1.0, 0)]
    assert np.all((fr >= 0) & (fr < 1))
    tiny = split_onsets([-1e-300, -2.0 ** -60, -7 - 2.0 ** -52])  # 1 - 1e-300 rounds to 1.0, no fraction: the position is the whole number above
    assert tiny[0].tolist() == [0, 0, -7] and tiny[1].tolist() == [0, 0, 0] and split_onsets([-2.0 ** -53])[1][0] == 1 - 2.0 ** -53
    rs = np.random.RandomState(3)
    p = rs.uniform(-1e6, 1e6, 1000)
    on, fr = split_onsets(p)
    assert np.array_equal(on + fr, p) and np.all((fr >= 0) & (fr < 1)) and d.split_onsets is split_onsets
    assert split_onsets([]) [0].shape == (0,) and split_onsets(np.int64([3, -4]))[1].tolist() == [0, 0]
    for bad in ([np.nan], [np.inf], [2.0 ** 63], [-2.0 ** 64]):
        with pytest.raises(ValueError, match="dusp-hip: positions are finite"):
            split_onsets(bad)


# ---- the planner and the kernel's text, under sanitizers ----------------------------------------------------------------------------------

def test_score_rows_plan_with_fractions_against_brute_force_under_sanitizers(tmp_path):
    """score_rows_plan of dusp_amd/csrc/score_plan.hpp with fracs (tests/native/score_rows_plan_frac_check.cpp lists what it covers)"""
    exe = str(tmp_path / "score_rows_plan_frac_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + SANITIZE + [os.path.join(ROOT, "tests", "native", "score_rows_plan_frac_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 6000 and rep["doubled"] >= 100 and rep["far_onsets"] >= 1000 and rep["tail_only"] >= 1000, rep
    assert rep["two_taps"] >= 10000 and rep["zero_fracs"] >= 100, rep


def test_score_frac_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/score_frac_engine.hip itself, compiled for the host with its lanes run one after the other, every row and the weight
    array a heap allocation of exactly its size, under AddressSanitizer and UBSan: a read of row[len] or row[-1] is caught here
    (tests/native/score_frac_kernel_check.cpp lists what it covers)."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "score_frac_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub"), "-x", "c++",
                           os.path.join(native, "score_frac_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 3000 and rep["doubled"] >= 100 and rep["windows"] >= 100, rep
    assert rep["two_taps"] > 1000000 and rep["tail_only"] >= 1000 and rep["whole_lists"] >= 100, rep


# ---- argument checks and refusal strings, Python and JavaScript, without a device ---------------------------------------------------------

SHAPE = "dusp-hip: fracs must have shape (voices=3,)"
FINITE = "dusp-hip: the fraction of voice 2 is not finite"
RANGE = "dusp-hip: the fraction of voice 1 is outside [0, 1)"
ONE_PART = "dusp-hip: the voices of a score are isomorphic circuits: a piece renders several instruments"
WHOLE = "dusp-hip: onsets are in samples, whole numbers: a fraction (or what is no number) is refused"


def python_refusals():
    import mix_voices
    d.configure(sv.SAMPLE_RATE)
    mono = lambda: [sv.voice(0), sv.voice(1), sv.voice(2)]
    two = lambda: [sv.voice(0), mix_voices.voice("filtered_saw", 0), sv.voice(1)]
    calls = {
        "shape": lambda: d.render_piece(mono(), [0, 1, 2], 0.01, 0.05, fracs=[0, 0]),
        "shapeScore": lambda: d.render_score(mono(), [0, 1, 2], 0.01, 0.05, fracs=[0, 0, 0, 0]),
        "finite": lambda: d.render_piece(mono(), [0, 1, 2], 0.01, 0.05, fracs=[0, 0.5, float("nan")]),
        "finitePcm": lambda: d.render_score_pcm(mono(), [0, 1, 2], 0.01, 0.05, fracs=[0, 0.5, float("inf")]),
        "finiteWav": lambda: d.render_score_wav(mono(), [0, 1, 2], 0.01, 0.05, pans=[0, 0, 0], fracs=[0, 0.5, float("-inf")]),
        "range": lambda: d.render_piece(mono(), [0, 1, 2], 0.01, 0.05, fracs=[0, 1, 0.5]),
        "rangePcm": lambda: d.render_piece_pcm(mono(), [0, 1, 2], 0.01, 0.05, fracs=[0, -0.5, 0.5]),
        "rangeWav": lambda: d.render_piece_wav(mono(), [0, 1, 2], 0.01, 0, pans=[0, 0, 0], fracs=[0.999, 1.5, 7]),
        "onePart": lambda: d.render_score(two(), [0, 1, 2], 0.01, 0.05, fracs=[0, 0, 0]),
    }
    got = {}
    for name, call in calls.items():
        with pytest.raises((ValueError, descriptor.DuspError)) as e:
            call()
        got[name] = str(e.value)
    return got


def test_python_refuses_by_string_before_anything_is_built():
    r = python_refusals()
    assert r["shape"] == r["shapeScore"] == SHAPE and r["finite"] == r["finitePcm"] == r["finiteWav"] == FINITE
    assert r["range"] == r["rangePcm"] == r["rangeWav"] == RANGE and r["onePart"] == ONE_PART
    with pytest.raises(ValueError) as e:  # (onsets stay whole numbers: the fraction travels beside them)
        d.render_piece([sv.voice(0), sv.voice(1), sv.voice(2)], [0, 0.5, 2], 0.01, 0.05, fracs=[0, 0.5, 0])
    assert str(e.value) == WHOLE
    a, b = np.zeros((1, 5), np.float32), np.zeros((1, 3), np.float32)
    for call in (lambda f: score_chain_rows([a, b], [0, 1], 9, fracs=f), lambda f: score_chain_rows_panned([a, b], [0, 1], [0, 0], 9, fracs=f)):
        for bad, message in (([0.5], "dusp-hip: fracs must have shape (voices=2,)"), ([0, np.nan], "dusp-hip: the fraction of voice 1 is not finite"),
                             ([1.0, 0], "dusp-hip: the fraction of voice 0 is outside [0, 1)"), ([0, -2.0 ** -60], "dusp-hip: the fraction of voice 1 is outside [0, 1)")):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(e.value) == message
        with pytest.raises(ValueError, match="onsets are whole numbers"):  # (onsets stay whole numbers: the fraction travels beside them)
            score_chain_rows([a, b], [0, 0.5], 9, fracs=[0, 0])
        assert call([0.5, np.nextafter(1.0, 0)]).shape[1] == 9
    fr = runtime.frac_arrays([0, 0.25, np.float32(0.5)], 3)
    assert fr.dtype == np.float64 and fr.flags.c_contiguous and fr.tolist() == [0, 0.25, 0.5]
    with pytest.raises(ValueError, match="voice_duration is one number"):
        d.render_score([sv.voice(0), sv.voice(1)], [0, 1], [0.01, 0.01], 0.05, fracs=[0, 0])
    # a timeline of no samples: nothing to render, checked all the same
    assert len(d.render_piece([sv.voice(0), sv.voice(1)], [0, 1], 0.01, 0, fracs=[0, 0.5])) == 0
    empty = d.render_piece_pcm([sv.voice(0), sv.voice(1)], [0, 1], 0.01, 0, pans=[0, 1], fracs=[0, 0.5])
    assert empty.data.shape == (0, 2) and d.render_piece_pcm([sv.voice(0), sv.voice(1)], [0, 1], 0.01, 0, fracs=[0, 0.5]).data.shape == (0, 1)
    # the symbols a binder looks for
    L = runtime.load()
    assert hasattr(L, "dusp_score_rows_frac_device") and hasattr(L, "dusp_render_host_score_parts_frac")


def test_the_javascript_host_refuses_with_pythons_strings():
    node = shutil.which("node")
    assert node is not None, "node is needed for the JavaScript host"
    addon = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")
    if not os.path.exists(addon):
        subprocess.check_call(["make", "-C", os.path.dirname(addon), "-s"])
    p = subprocess.run([node, os.path.join(ROOT, "tests", "js", "check_frac.js"), "--sampleRate=48000", "refusals"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    assert rep["refusals"] == python_refusals(), rep["refusals"]
    assert rep["addonCall"] is True and rep["whole"] == "dusp-hip: renderPiece: onsets are in samples, whole numbers: a fraction is refused"
    assert rep["splitTiny"] == [0, 0] and rep["splitBad"] == "dusp-hip: positions are finite numbers of samples within int64"
    positions = [0, 5, -5, 5538.46153846, -0.25, -3.75, 1 / 3, 2.0 ** 51 + 0.5, -(2.0 ** 40) - 0.125]
    on, fr = split_onsets(positions)
    assert rep["split"]["onsets"] == on.tolist() and rep["split"]["fracs"] == fr.tolist()
