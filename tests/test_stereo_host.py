"""Stereo pieces, on the CPU: dusp_amd.mix.score_chain_rows_stereo — score_chain_rows over voices that are panned mono rows, plain mono
rows or rows of two channels, the kind a property of the voice — over the oracle's per-voice renders IS the oracle's render of
`Sum.many(Delay(P_k, onset_k + frac_k, maxDelay))` as one circuit, P_k = Pan(Multiply(v_k, g_k), p_k) or Multiply(v_k, g_k), bit for bit
on both channels, in three orders of the voice list.  Then the chain's algebra on planted rows, the kernel's text on the host under
sanitizers (tests/native/score_stereo_kernel_check.cpp), and the argument checks and refusal strings of the Python and the JavaScript
host, which need no device."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import score_voices as sv
import stereo_cases as sc
from conftest import ROOT
from dusp_amd import descriptor, render, runtime
from dusp_amd.mix import score_chain_rows, score_chain_rows_panned, score_chain_rows_stereo
from test_piece_host import SANITIZE, bits, same

NT = 1301
N_PLANTED = 13


def oracle_whole(oracle, n, order, with_gains, with_fracs):
    """-> (the oracle's per-voice renders, its render of the whole piece as one circuit [2, sv.NT], onsets, fracs, gains, pans)"""
    d.configure(sv.SAMPLE_RATE)
    onsets, fracs, gains = sc.layout(n, with_fracs)
    g = gains if with_gains else None
    pans = sc.stereo_pans(n, order)
    rows = [np.asarray(oracle.render(descriptor.extract(v).words, sv.NV), dtype=np.float32) for v in sc.voices_for(n, order)]
    assert [r.shape for r in rows] == [(2 if kind == sc.TWO else 1, sv.NV) for kind in sc.kinds_for(n, order)]
    want = np.asarray(oracle.render(descriptor.extract(sc.as_one_stereo_circuit(sc.voices_for(n, order), onsets, pans, g, fracs)).words, sv.NT), dtype=np.float32)
    if want.shape[0] == 1:  # (a lone plain mono voice: the reference's circuit is mono, and the stereo timeline hears it alike on both channels)
        assert n == 1 and sc.kinds_for(n, order) == [sc.MONO]
        want = np.concatenate([want, want])
    return rows, want, onsets, fracs, g, pans


@pytest.mark.parametrize("with_fracs", [False, True], ids=["whole", "fracs"])
@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("n", [1, 2, 13, 37])
def test_the_stereo_chain_over_the_voices_renders_is_sum_many_of_the_mixed_piece(n, order, with_gains, with_fracs, oracle):
    rows, want, onsets, fracs, g, pans = oracle_whole(oracle, n, order, with_gains, with_fracs)
    assert want.shape == (2, sv.NT) and np.abs(want).max() > 0
    if n >= 13:
        assert not np.array_equal(want[0], want[1]) and {r.shape[0] for r in rows} == {1, 2} and np.isnan(pans).any() and np.isfinite(pans).any()
    if with_fracs and n > 1:
        assert (fracs != 0).any() and (fracs == 0).any()
    got = score_chain_rows_stereo(rows, onsets, pans, sv.NT, None, g, fracs=fracs)
    assert got.dtype == np.float32 and got.shape == (2, sv.NT)
    assert np.array_equal(bits(got), bits(want)), "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0)))


# ---- the chain's algebra on planted rows ------------------------------------------------------------------------------------------------

def test_the_planted_rows_hold_what_they_are_built_to_hold():
    rows, onsets, lengths, gains, pans, init, fracs = sc.planted(N_PLANTED)
    assert {r.shape[1] for r in rows} == {773, 1, 255, 0, 257, 3} and [r.shape[0] for r in rows] == [1, 1, 2] * 4 + [1]
    assert np.array_equal(np.isfinite(pans), np.arange(N_PLANTED) % 3 == 0) and np.isnan(pans[~np.isfinite(pans)]).all()
    assert (onsets < 0).any() and (onsets + lengths > NT).any() and (lengths == 0).any()
    assert {0.0, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -53} <= set(fracs.tolist())
    raw, cooked = score_chain_rows_stereo(rows, onsets, pans, NT, lengths, raw=True), score_chain_rows_stereo(rows, onsets, pans, NT, lengths)
    assert np.isnan(raw).any() and not np.isnan(cooked).any() and np.isinf(cooked).any() and not np.array_equal(bits(cooked[0]), bits(cooked[1]))
    edge, edge_onsets, edge_pans = sc.edge_rows()
    assert [r.shape for r in edge[:2]] == [(2, 0), (2, 1)]
    got = score_chain_rows_stereo(edge, edge_onsets, edge_pans, 8)
    assert got.tolist() == [[0, 0, 0, 1, 3.5, 3, 0, 0], [0, 0, 0, 1, -0.5, 3, 0, 0]]


@pytest.mark.parametrize("with_fracs", [False, True], ids=["whole", "fracs"])
def test_one_kind_of_voice_gives_the_bits_of_the_chain_of_that_kind(with_fracs):
    for kw in ({}, {"gains": True}, {"init": True, "raw": True}, {"gains": True, "init": True}):
        def args(planted):
            rows, onsets, lengths, gains, pans, init, fracs = planted
            extra = {"gains": gains if kw.get("gains") else None, "init": init if kw.get("init") else None, "raw": kw.get("raw", False), "fracs": fracs if with_fracs else None}
            return rows, onsets, lengths, pans, extra
        rows, onsets, lengths, pans, extra = args(sc.planted(N_PLANTED, NT, sc.PANNED))
        assert all(r.shape[0] == 1 for r in rows) and np.isfinite(pans).all()
        assert same(score_chain_rows_stereo(rows, onsets, pans, NT, lengths, **extra), score_chain_rows_panned(rows, onsets, pans, NT, lengths, **extra)), kw
        rows, onsets, lengths, pans, extra = args(sc.planted(N_PLANTED, NT, sc.TWO))
        assert all(r.shape[0] == 2 for r in rows) and np.isnan(pans).all()
        assert same(score_chain_rows_stereo(rows, onsets, pans, NT, lengths, **extra), score_chain_rows(rows, onsets, NT, lengths, **extra)), kw
        assert same(score_chain_rows_stereo(rows, onsets, None, NT, lengths, **extra), score_chain_rows(rows, onsets, NT, lengths, **extra)), kw
        # plain mono rows: the mono chain, heard alike on both channels (each continuing its own channel of init)
        rows, onsets, lengths, pans, extra = args(sc.planted(N_PLANTED, NT, sc.MONO))
        got = score_chain_rows_stereo(rows, onsets, pans, NT, lengths, **extra)
        for c in (0, 1):
            mono = dict(extra, init=None if extra["init"] is None else extra["init"][c:c + 1])
            assert same(got[c:c + 1], score_chain_rows(rows, onsets, NT, lengths, **mono)), (kw, c)


@pytest.mark.parametrize("with_fracs", [False, True], ids=["whole", "fracs"])
@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
def test_a_stereo_chain_cut_at_every_voice_and_continued_is_the_same_chain(with_gains, with_fracs):
    rows, onsets, lengths, gains, pans, _, fracs = sc.planted(N_PLANTED)
    n = len(rows)
    g, f = gains if with_gains else None, fracs if with_fracs else None
    cut_of = lambda a, lo, hi: None if a is None else a[lo:hi]
    whole_raw, whole = (score_chain_rows_stereo(rows, onsets, pans, NT, lengths, g, raw=raw, fracs=f) for raw in (True, False))
    for cut in range(0, n + 1):
        head = (score_chain_rows_stereo(rows[:cut], onsets[:cut], pans[:cut], NT, lengths[:cut], cut_of(g, 0, cut), raw=True, fracs=cut_of(f, 0, cut)) if cut
                else np.zeros((2, NT), dtype=np.float32))
        for raw, want in ((True, whole_raw), (False, whole)):
            got = score_chain_rows_stereo(rows[cut:], onsets[cut:], pans[cut:], NT, lengths[cut:], cut_of(g, cut, n), init=head, raw=raw, fracs=cut_of(f, cut, n))
            assert same(got, want), (cut, raw)
    # a -0 partial sum survives voices that do not cover the sample, and leaves as +0: nothing is added outside a span, not even a zero
    uncovered = np.ones(NT, dtype=bool)
    for k in range(n):
        uncovered[max(int(onsets[k]), 0):max(int(onsets[k] + lengths[k]) + 1, 0)] = False
    assert uncovered.any()
    init = np.full((2, NT), -0.0, dtype=np.float32)
    cont = score_chain_rows_stereo(rows, onsets, pans, NT, lengths, g, init=init, raw=True, fracs=f)
    assert np.signbit(cont[:, uncovered]).all() and (cont[:, uncovered] == 0).all()
    assert not np.signbit(score_chain_rows_stereo(rows, onsets, pans, NT, lengths, g, init=init, fracs=f)[:, uncovered]).any()


@pytest.mark.parametrize("with_fracs", [False, True], ids=["whole", "fracs"])
def test_the_stereo_timeline_cut_into_windows_is_the_whole(with_fracs):
    rows, onsets, lengths, gains, pans, _, fracs = sc.planted(N_PLANTED)
    f = fracs if with_fracs else None
    for raw in (True, False):
        whole = score_chain_rows_stereo(rows, onsets, pans, NT, lengths, gains, raw=raw, fracs=f)
        for cut in (1, 13, 256, 899, 1300):
            first = score_chain_rows_stereo(rows, onsets, pans, cut, lengths, gains, raw=raw, fracs=f)
            second = score_chain_rows_stereo(rows, onsets - cut, pans, NT - cut, lengths, gains, raw=raw, fracs=f)  # (onsets shifted: many are negative now)
            assert same(np.concatenate([first, second], axis=1), whole), (raw, cut)


def test_stereo_argument_shapes_are_checked():
    a, b, w = np.zeros((1, 5), np.float32), np.zeros((1, 3), np.float32), np.zeros((2, 4), np.float32)
    call = score_chain_rows_stereo
    nan = float("nan")
    for bad in (lambda: call([a, np.zeros((3, 3), np.float32)], [0, 1], None, 9), lambda: call([a, np.zeros(3, np.float32)], [0, 1], None, 9),
                lambda: call([a, w], [0, 1], [0, 0.5], 9), lambda: call([a, w], [0, 1], [0], 9), lambda: call([a, b], [0, 1], [np.inf, nan], 9),
                lambda: call([a, b], [0, 1], [0, nan], 9, comp=[1.0]), lambda: call([a, w], [0], None, 9), lambda: call([a, w], [0, 1], None, 9, lengths=[5, 5]),
                lambda: call([a, w], [0, 1], None, 9, gains=[1]), lambda: call([a, w], [0, 1], None, 9, init=np.zeros((1, 9))), lambda: call([a, w], [0, 0.5], None, 9),
                lambda: call([a, w], [0, 1], None, -1), lambda: call([a, w], [0, 1], None, 9, fracs=[0, 1.0])):
        with pytest.raises(ValueError, match="dusp-hip"):
            bad()
    assert call([a, w, b], [0, 1, 2], [0.5, None, nan], 9, lengths=[5, 3, 3]).shape == (2, 9) and call([], [], None, 4).shape == (2, 4) and call([], [], [], 4).shape == (2, 4)
    with pytest.raises(ValueError) as e:
        call([a, w], [0, 1], [0, 0.5], 9)
    assert str(e.value) == TWO_PANNED % 1
    with pytest.raises(ValueError) as e:
        call([a, np.zeros((3, 3), np.float32)], [0, 1], None, 9)
    assert str(e.value) == CHANNELS % (1, 3)


# ---- the kernel's text, under sanitizers --------------------------------------------------------------------------------------------------

def test_score_stereo_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/score_stereo_engine.hip itself, compiled for the host with its lanes run one after the other, every row a heap
    allocation of exactly channels x samples floats, under AddressSanitizer and UBSan (tests/native/score_stereo_kernel_check.cpp lists
    what it covers); and the plan without row_channels is the plan it was."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "score_stereo_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub"), "-x", "c++",
                           os.path.join(native, "score_stereo_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 5000 and rep["doubled"] >= 100 and rep["windows"] >= 100 and rep["zero_first"] >= 1000, rep
    assert rep["frac_launches"] >= 1000 and rep["mixed_batches"] >= 1000 and rep["plans_same"] == rep["cases"], rep


# ---- argument checks and refusal strings, Python and JavaScript, without a device ---------------------------------------------------------

ONE_NUMBER = "dusp-hip: the voices of a piece must have one number of output channels: part 1 has 2, part 0 has 1"
TWO_PANNED = "dusp-hip: a two-channel voice is not panned: the pan of voice %d must be NaN (not placed)"
CHANNELS = "dusp-hip: a voice of a stereo piece has one or two channels: voice %d has %d"
SHAPE = "dusp-hip: pans must have shape (voices=3,)"
FINITE = "dusp-hip: the pan of voice 2 is not finite"
NO_PLACES = runtime.STEREO_NO_PLACES


def wide_voice(k):
    return sc.voice(k, sc.TWO)


def three_channel_voice(k):
    return d.Multiply(sv.voice(k), [0.5, 0.25, 0.125])


def python_refusals():
    d.configure(sv.SAMPLE_RATE)
    mixed = lambda: [sv.voice(0), wide_voice(1), sv.voice(2)]
    calls = {
        "withoutStereo": lambda: d.render_piece(mixed(), [0, 1, 2], 0.01, 0.05),
        "twoPanned": lambda: d.render_piece(mixed(), [0, 1, 2], 0.01, 0.05, pans=[0, 0.5, None], stereo=True),
        "twoPannedPcm": lambda: d.render_piece_pcm(mixed(), [0, 1, 2], [0.01, 0.02, 0.01], 0.05, pans=[None, -1, None], stereo=True),
        "twoPannedWav": lambda: d.render_piece_wav(mixed(), [0, 1, 2], 0.01, 0, pans=[0, 0, 0], stereo=True),
        "twoPannedScore": lambda: d.render_score([wide_voice(0), wide_voice(1), wide_voice(2)], [0, 1, 2], 0.01, 0.05, pans=[None, 0.25, None], stereo=True),
        "channels": lambda: d.render_piece([sv.voice(0), wide_voice(1), three_channel_voice(2)], [0, 1, 2], 0.01, 0.05, stereo=True),
        "shape": lambda: d.render_piece(mixed(), [0, 1, 2], 0.01, 0.05, pans=[0, None], stereo=True),
        "finite": lambda: d.render_piece(mixed(), [0, 1, 2], 0.01, 0.05, pans=[0, None, float("inf")], stereo=True),
        "finiteWav": lambda: d.render_score_wav([sv.voice(0), sv.voice(1), sv.voice(2)], [0, 1, 2], 0.01, 0.05, pans=[0, None, 1e39], stereo=True),
        "places": lambda: d.render_piece(mixed(), [0, 1, 2], 0.01, 0.05, places=[[0, 1]] * 3, stereo=True),
        "placesScorePcm": lambda: d.render_score_pcm([sv.voice(0), sv.voice(1), sv.voice(2)], [0, 1, 2], 0.01, 0.05, places=[[0, 1]] * 3, stereo=True),
    }
    got = {}
    for name, call in calls.items():
        with pytest.raises((ValueError, descriptor.DuspError)) as e:
            call()
        got[name] = str(e.value)
    return got


def test_python_refuses_by_string_before_anything_is_built():
    r = python_refusals()
    assert r["withoutStereo"] == ONE_NUMBER  # (without the keyword nothing has changed)
    assert r["twoPanned"] == r["twoPannedPcm"] == r["twoPannedWav"] == r["twoPannedScore"] == TWO_PANNED % 1
    assert r["channels"] == CHANNELS % (2, 3) and r["shape"] == SHAPE and r["finite"] == r["finiteWav"] == FINITE
    assert r["places"] == r["placesScorePcm"] == NO_PLACES
    assert render.check_stereo_channels([1, 2], [0, 1, 0], np.array([0.5, np.nan, np.nan], dtype=np.float32)) == 2
    pans, comp = runtime.stereo_pan_arrays([-1, None, float("nan"), 0.3], 4)
    assert pans.dtype == np.float32 and comp.dtype == np.float64 and np.array_equal(np.isnan(pans), [False, True, True, False])
    assert comp[0] == 1.0 and comp[3] == runtime.pan_comp(np.float32([0.3]))[0] and np.isnan(runtime.stereo_pan_arrays(None, 3)[0]).all()
    # a timeline of no samples: nothing to render, checked all the same
    mixed = [sv.voice(0), wide_voice(1)]
    assert len(d.render_piece(mixed, [0, 1], 0.01, 0, stereo=True)) == 0
    empty = d.render_piece_pcm([sv.voice(0), wide_voice(1)], [0, 1], 0.01, 0, pans=[0.5, None], stereo=True)
    assert empty.data.shape == (0, 2) and empty.numberOfChannels == 2
    # the symbols a binder looks for
    L = runtime.load()
    assert hasattr(L, "dusp_score_rows_stereo_device") and hasattr(L, "dusp_render_host_score_parts_stereo")


def test_the_javascript_host_refuses_with_pythons_strings():
    node = shutil.which("node")
    assert node is not None, "node is needed for the JavaScript host"
    addon = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")
    if not os.path.exists(addon):
        subprocess.check_call(["make", "-C", os.path.dirname(addon), "-s"])
    p = subprocess.run([node, os.path.join(ROOT, "tests", "js", "check_stereo.js"), "--sampleRate=48000", "refusals"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    assert rep["refusals"] == python_refusals(), rep["refusals"]
    assert rep["addonCall"] is True
    pans = runtime.stereo_pan_arrays([-1, None, float("nan"), 0.3, 1e-40], 5)[0]
    got = np.array([np.nan if p is None else p for p in rep["pans"]], dtype=np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(pans)) and np.array_equal(got[~np.isnan(got)].view(np.uint32), pans[~np.isnan(pans)].view(np.uint32))
