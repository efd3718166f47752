"""Stereo placement, on the CPU: dusp_amd.mix.score_chain_rows_panned — score_chain_rows over MONO rows with the reference's Pan unit
applied where a voice is added — over the oracle's mono renders IS the oracle's render of
`Sum.many(Delay(Pan(Multiply(voice_k, g_k), pan_k), onset_k, maxDelay))` as one circuit, bit for bit on both channels.  Then the chain's
algebra on planted mono rows, the kernel's text on the host under sanitizers (tests/native/score_pan_kernel_check.cpp), and the argument
checks and refusal strings of the Python and the JavaScript host, which need no device."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import mix_voices
import score_voices as sv
from conftest import ROOT
from dusp_amd import descriptor, render, runtime
from dusp_amd.mix import pan_comp, score_chain_rows, score_chain_rows_panned
from pan_cases import FIXED_PANS, as_one_panned_circuit, pans_for, planted
from test_piece_host import FMAX, NV_SAW, SANITIZE, bits, interleaved_voice, oracle_rows, same


def assert_bits(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape == (2, sv.NT)
    assert np.array_equal(bits(got), bits(want)), "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0)))


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("n", [2, 13, 37])
def test_the_panned_chain_over_mono_renders_is_sum_many_of_delayed_pans(n, with_gains, oracle):
    d.configure(sv.SAMPLE_RATE)
    onsets, _, gains = sv.layout(n)
    g = gains if with_gains else None
    pans = pans_for(n)
    assert pans[0] == -1 and (n < 3 or (pans[1] == 1 and pans[2] == 0)) and np.all(np.abs(pans) <= 1)
    rows = [np.asarray(oracle.render(descriptor.extract(sv.voice(k)).words, sv.NV), dtype=np.float32) for k in range(n)]
    assert all(r.shape == (1, sv.NV) for r in rows)
    circuit = as_one_panned_circuit([sv.voice(k) for k in range(n)], onsets, pans, g)
    want = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
    assert want.shape == (2, sv.NT) and np.abs(want).max() > 0 and not np.array_equal(want[0], want[1])
    assert_bits(score_chain_rows_panned(rows, onsets, pans, sv.NT, None, g), want)
    assert_bits(score_chain_rows_panned(rows, onsets, pans, sv.NT, None, g, comp=[math.pow(10, ((1 - abs(float(p))) * 1.5) / 20) for p in pans]), want)


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("n", [2, 13, 37])
def test_the_panned_chain_over_the_parts_renders_is_the_interleaved_piece(n, with_gains, oracle):
    rows = oracle_rows(n, oracle)  # (773 and 1031 samples in turn, rendered part by part)
    assert [r.shape for r in rows] == [(1, sv.NV if k % 2 == 0 else NV_SAW) for k in range(n)]
    onsets, _, gains = sv.layout(n)
    g = gains if with_gains else None
    pans = pans_for(n)
    d.configure(sv.SAMPLE_RATE)
    circuit = as_one_panned_circuit([interleaved_voice(k) for k in range(n)], onsets, pans, g)
    want = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
    assert_bits(score_chain_rows_panned(rows, onsets, pans, sv.NT, None, g), want)


# ---- the chain's algebra on planted rows ------------------------------------------------------------------------------------------------

N_PLANTED = 13


def test_the_planted_rows_hold_what_they_are_built_to_hold():
    rows, onsets, lengths, gains, pans, init = planted(N_PLANTED)
    assert {r.shape[1] for r in rows} == {773, 1, 255, 0, 257, 3} and all(r.shape[0] == 1 for r in rows)
    assert set(pans.tolist()) == set(np.array(FIXED_PANS, dtype=np.float32).tolist()) and 0 < pans[3] < np.finfo(np.float32).tiny
    assert (onsets < 0).any() and (onsets + lengths > 1301).any() and (lengths == 0).any()
    raw, cooked = score_chain_rows_panned(rows, onsets, pans, 1301, lengths, raw=True), score_chain_rows_panned(rows, onsets, pans, 1301, lengths)
    assert np.isnan(raw).any() and not np.isnan(cooked).any() and np.isinf(cooked).any() and not np.array_equal(bits(cooked[0]), bits(cooked[1]))


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
def test_a_panned_chain_cut_at_every_voice_and_continued_is_the_same_chain(with_gains):
    rows, onsets, lengths, gains, pans, _ = planted(N_PLANTED)
    n, n_total = len(rows), 1301
    g = gains if with_gains else None
    whole_raw, whole = score_chain_rows_panned(rows, onsets, pans, n_total, lengths, g, raw=True), score_chain_rows_panned(rows, onsets, pans, n_total, lengths, g)
    for cut in range(0, n + 1):
        head = (score_chain_rows_panned(rows[:cut], onsets[:cut], pans[:cut], n_total, lengths[:cut], None if g is None else g[:cut], raw=True) if cut
                else np.zeros((2, n_total), dtype=np.float32))
        for raw, want in ((True, whole_raw), (False, whole)):
            got = score_chain_rows_panned(rows[cut:], onsets[cut:], pans[cut:], n_total, lengths[cut:], None if g is None else g[cut:], init=head, raw=raw)
            assert same(got, want), (cut, raw)
    # a -0 partial sum survives voices that do not cover the sample, and leaves as +0: nothing is added outside a span, not even a zero
    uncovered = np.ones(n_total, dtype=bool)
    for k in range(n):
        uncovered[max(int(onsets[k]), 0):max(int(onsets[k] + lengths[k]), 0)] = False
    assert uncovered.any()
    init = np.full((2, n_total), -0.0, dtype=np.float32)
    cont = score_chain_rows_panned(rows, onsets, pans, n_total, lengths, g, init=init, raw=True)
    assert np.signbit(cont[:, uncovered]).all() and (cont[:, uncovered] == 0).all()
    assert not np.signbit(score_chain_rows_panned(rows, onsets, pans, n_total, lengths, g, init=init)[:, uncovered]).any()


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
def test_the_panned_timeline_cut_into_windows_is_the_whole(with_gains):
    rows, onsets, lengths, gains, pans, _ = planted(N_PLANTED)
    g = gains if with_gains else None
    for raw in (True, False):
        whole = score_chain_rows_panned(rows, onsets, pans, 1301, lengths, g, raw=raw)
        for cut in (1, 13, 256, 899, 1300):
            first = score_chain_rows_panned(rows, onsets, pans, cut, lengths, g, raw=raw)
            second = score_chain_rows_panned(rows, onsets - cut, pans, 1301 - cut, lengths, g, raw=raw)  # (onsets shifted: many are negative now)
            assert same(np.concatenate([first, second], axis=1), whole), (raw, cut)


def test_centred_voices_with_a_compensation_of_two_are_score_chain_rows_on_both_channels():
    """pan 0 and comp 2: ((x * 1) / 2) * 2 is x itself, so both channels are the mono chain"""
    rows, onsets, lengths, gains, _, init = planted(N_PLANTED)
    zeros, twos = np.zeros(len(rows), dtype=np.float32), np.full(len(rows), 2.0)
    for kw, mono_kw in (({}, {}), ({"lengths": lengths, "gains": gains}, {"lengths": lengths, "gains": gains}), ({"lengths": lengths, "raw": True}, {"lengths": lengths, "raw": True})):
        got = score_chain_rows_panned(rows, onsets, zeros, 1301, comp=twos, **kw)
        mono = score_chain_rows(rows, onsets, 1301, **mono_kw)
        assert mono.shape == (1, 1301) and same(got[0:1], mono) and same(got[1:2], mono), sorted(kw)
    for c in (0, 1):  # with init: each channel continues its own
        got = score_chain_rows_panned(rows, onsets, zeros, 1301, lengths, gains, init=init, comp=twos)
        assert same(got[c:c + 1], score_chain_rows(rows, onsets, 1301, lengths, gains, init=init[c:c + 1]))


def test_subnormal_and_overflowing_terms_come_out_as_numpy_gives_them():
    f32, f64 = np.float32, np.float64
    x = np.array([[5e-39, FMAX, -FMAX, 1e-45]], dtype=f32)
    with np.errstate(all="ignore"):
        # centre: (x * 1 / 2) * 10^(1.5/20); 5e-39 lands in the f32 subnormal range, 1e-45 (the smallest subnormal) rounds there too
        comp0 = math.pow(10, 1.5 / 20)
        got = score_chain_rows_panned([x], [0], [0.0], 4, raw=True)
        want = ((x[0].astype(f64) * f64(1) / f64(2)) * f64(comp0)).astype(f32)
        assert np.array_equal(bits(got[0]), bits(want)) and np.array_equal(bits(got[1]), bits(want))
        assert 0 < got[0, 0] < np.finfo(f32).tiny and got[0, 0] == f32((f64(x[0, 0]) / 2) * comp0)
        # hard left: the left channel takes x * 2 / 2 * 1 = x — FMAX * 2 is no overflow in f64 — and the right x * 0, a signed zero:
        # added to the chain's +0 it is +0, and continued from a -0 it keeps the sign where the term's is negative
        got = score_chain_rows_panned([x], [0], [-1.0], 4, raw=True)
        assert np.array_equal(bits(got[0]), bits(x[0])) and np.array_equal(bits(got[1]), bits(np.zeros(4, dtype=f32)))
        got = score_chain_rows_panned([x], [0], [-1.0], 4, init=np.full((2, 4), -0.0, dtype=f32), raw=True)
        assert np.array_equal(bits(got[0]), bits(x[0])) and np.array_equal(bits(got[1]), bits(np.array([0.0, 0.0, -0.0, 0.0], dtype=f32)))
        # outside [-1, 1], not clamped: at 1.5 the right channel takes FMAX * 2.5 / 2 * 10^(-0.0375) = 1.147 FMAX: infinite in f32
        got = score_chain_rows_panned([x], [0], [1.5], 4, raw=True)
        comp = math.pow(10, ((1 - 1.5) * 1.5) / 20)
        assert np.isposinf(got[1, 1]) and np.isneginf(got[1, 2]) and got[0, 1] == f32(((f64(FMAX) * -0.5) / 2) * comp) and np.isfinite(got[0, 1]) and got[0, 1] < 0
        # two such terms on one sample: inf + -inf is NaN raw, +0 delivered
        both = score_chain_rows_panned([x[:, 1:2], x[:, 2:3]], [0, 0], [1.5, 1.5], 1, raw=True)
        assert np.isnan(both[1, 0]) and score_chain_rows_panned([x[:, 1:2], x[:, 2:3]], [0, 0], [1.5, 1.5], 1)[1, 0] == 0
    assert np.array_equal(pan_comp(np.array(FIXED_PANS, dtype=f32)), [math.pow(10, ((1 - abs(float(f32(p)))) * 1.5) / 20) for p in FIXED_PANS])


def test_panned_argument_shapes_are_checked():
    a, b = np.zeros((1, 5), np.float32), np.zeros((1, 3), np.float32)
    call = score_chain_rows_panned
    for bad in (lambda: call([a, np.zeros((2, 3), np.float32)], [0, 1], [0, 0], 9), lambda: call([a, np.zeros(3, np.float32)], [0, 1], [0, 0], 9),
                lambda: call([a, b], [0, 1], [0], 9), lambda: call([a, b], [0, 1], [0, np.nan], 9), lambda: call([a, b], [0, 1], [np.inf, 0], 9),
                lambda: call([a, b], [0, 1], [0, 0], 9, comp=[1.0]), lambda: call([a, b], [0], [0, 0], 9), lambda: call([a, b], [0, 1], [0, 0], 9, lengths=[5, 4]),
                lambda: call([a, b], [0, 1], [0, 0], 9, gains=[1]), lambda: call([a, b], [0, 1], [0, 0], 9, init=np.zeros((1, 9))), lambda: call([a, b], [0, 0.5], [0, 0], 9),
                lambda: call([a, b], [0, 1], [0, 0], -1)):
        with pytest.raises(ValueError, match="dusp-hip"):
            bad()
    assert call([a, b], [0, 1], [0.5, 7.0], 9, lengths=[5, 3]).shape == (2, 9) and call([], [], [], 4).shape == (2, 4)


# ---- the kernel's text, under sanitizers --------------------------------------------------------------------------------------------------

def test_score_pan_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/score_pan_engine.hip itself, compiled for the host with its lanes run one after the other, every row a heap
    allocation of exactly its size, under AddressSanitizer and UBSan; and the identity (y / 2) * comp == y * (comp / 2) the kernel's
    coefficients rest on (tests/native/score_pan_kernel_check.cpp lists what it covers)."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "score_pan_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub"), "-x", "c++",
                           os.path.join(native, "score_pan_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 3000 and rep["doubled"] >= 100 and rep["windows"] >= 100 and rep["zero_first"] >= 1000, rep
    assert rep["identity_bad"] == 0 and rep["identity"] > 1000000, rep


# ---- argument checks and refusal strings, Python and JavaScript, without a device ---------------------------------------------------------

MONO = "dusp-hip: a panned voice is mono: part 1 has 2 output channels"
SHAPE = "dusp-hip: pans must have shape (voices=3,)"
FINITE = "dusp-hip: the pan of voice 2 is not finite"
ONE_PART = "dusp-hip: the voices of a score are isomorphic circuits: a piece renders several instruments"


def python_refusals():
    d.configure(sv.SAMPLE_RATE)
    mixed = lambda: [sv.voice(0), mix_voices.voice("pan", 0), sv.voice(1)]
    mono = lambda: [sv.voice(0), sv.voice(1), sv.voice(2)]
    two = lambda: [sv.voice(0), mix_voices.voice("filtered_saw", 0), sv.voice(1)]
    calls = {
        "mono": lambda: d.render_piece(mixed(), [0, 1, 2], 0.01, 0.05, pans=[0, 0, 0]),
        "monoPcm": lambda: d.render_piece_pcm(mixed(), [0, 1, 2], [0.01, 0.02, 0.01], 0.05, pans=[0, 0, 0]),
        "monoWav": lambda: d.render_piece_wav(mixed(), [0, 1, 2], 0.01, 0, pans=[0, 0, 0]),
        "shape": lambda: d.render_piece(mono(), [0, 1, 2], 0.01, 0.05, pans=[0, 0]),
        "shapeScore": lambda: d.render_score(mono(), [0, 1, 2], 0.01, 0.05, pans=[0, 0, 0, 0]),
        "finite": lambda: d.render_piece(mono(), [0, 1, 2], 0.01, 0.05, pans=[0, 0.5, float("nan")]),
        "finitePcm": lambda: d.render_score_pcm(mono(), [0, 1, 2], 0.01, 0.05, pans=[0, 0.5, float("inf")]),
        "finiteWav": lambda: d.render_score_wav(mono(), [0, 1, 2], 0.01, 0.05, pans=[0, 0.5, 1e39]),  # (no f32 holds 1e39: infinite)
        "onePart": lambda: d.render_score(two(), [0, 1, 2], 0.01, 0.05, pans=[0, 0, 0]),
    }
    got = {}
    for name, call in calls.items():
        with pytest.raises((ValueError, descriptor.DuspError)) as e:
            call()
        got[name] = str(e.value)
    return got


def test_python_refuses_by_string_before_anything_is_built():
    r = python_refusals()
    assert r["mono"] == r["monoPcm"] == r["monoWav"] == MONO
    assert r["shape"] == SHAPE and r["shapeScore"] == SHAPE and r["finite"] == r["finitePcm"] == r["finiteWav"] == FINITE and r["onePart"] == ONE_PART
    with pytest.raises(descriptor.DuspError) as e:
        render.check_pan_channels([1, 2, 1])
    assert str(e.value) == MONO and render.check_pan_channels([1, 1]) == 2
    pans, comp = runtime.pan_arrays([-1, 0.3, 1.5], 3)
    assert pans.dtype == np.float32 and comp.dtype == np.float64 and comp[0] == 1.0 and np.array_equal(comp, pan_comp(pans))
    with pytest.raises(ValueError, match="voice_duration is one number"):
        d.render_score([sv.voice(0), sv.voice(1)], [0, 1], [0.01, 0.01], 0.05, pans=[0, 0])
    # a timeline of no samples: nothing to render, checked all the same
    assert len(d.render_piece([sv.voice(0), sv.voice(1)], [0, 1], 0.01, 0, pans=[0, 1])) == 0
    empty = d.render_piece_pcm([sv.voice(0), sv.voice(1)], [0, 1], 0.01, 0, pans=[0, 1])
    assert empty.data.shape == (0, 2) and empty.numberOfChannels == 2
    # the symbols a binder looks for
    L = runtime.load()
    assert hasattr(L, "dusp_score_rows_pan_device") and hasattr(L, "dusp_render_host_score_parts_pan")


def test_the_javascript_host_refuses_with_pythons_strings():
    node = shutil.which("node")
    assert node is not None, "node is needed for the JavaScript host"
    addon = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")
    if not os.path.exists(addon):
        subprocess.check_call(["make", "-C", os.path.dirname(addon), "-s"])
    p = subprocess.run([node, os.path.join(ROOT, "tests", "js", "check_pan.js"), "--sampleRate=48000", "refusals"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    assert rep["refusals"] == python_refusals(), rep["refusals"]
    assert rep["check"] == MONO and rep["checkOk"] == 2 and rep["addonCall"] is True
    pans, comp = runtime.pan_arrays(FIXED_PANS + [0.7, -0.123456789], len(FIXED_PANS) + 2)
    assert np.array_equal(np.array(rep["pans"], dtype=np.float32).view(np.uint32), pans.view(np.uint32))
    # Math.pow and math.pow are two implementations of one function: each host passes its own, and they agree to an ulp here
    assert np.all(np.abs(np.array(rep["comp"]) - comp) <= np.spacing(comp))
