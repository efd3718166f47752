"""Loudness delivery in the JavaScript host (dusp_amd/js): the refusal strings and what a call over no samples resolves to are
Python's — compared without a device — and, on the GPU, the true peaks, the gain, the level and the frames of renderPiece /
renderPiecePcm / renderPieceWav with truePeak and loudness, and of truePeak(), are what Python's calls return: both hosts hand on what
the library computed (tests/js/check_loudness.js)."""
import hashlib
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
import track_cases as tc
from conftest import ROOT
from dusp_amd import mix, render, wav
from pan_cases import pans_for

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")


def node(*args):
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_loudness.js"), "--sampleRate=48000"] + list(args), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    return rep


def num(x):
    x = float(x)
    return x if math.isfinite(x) else {"inf": "Infinity", "-inf": "-Infinity", "nan": "NaN"}[str(x)]


def plain(meters):
    """a render.Meters with true peaks as tests/js/check_loudness.js writes one"""
    return {"names": meters.names, "lufs": [num(meters.lufs[k]) for k in meters.names], "rms": [[num(v) for v in meters.rms[k]] for k in meters.names],
            "truePeak": [[num(v) for v in meters.true_peak[k]] for k in meters.names]}


def sha(data):
    return hashlib.sha256(data if isinstance(data, bytes) else np.ascontiguousarray(data).tobytes()).hexdigest()


def test_the_refusals_and_the_empty_results_are_pythons():
    rep = node("surface")
    calls = {"renderPiece", "renderScore", "renderPiecePcm", "renderScorePcm", "renderPieceWav", "renderScoreWav"}
    assert set(rep["notBool"]) == calls and all(messages == [mix.TRUE_PEAK_NOT_BOOL] * 2 + [mix.METERS_NOT_BOOL] for messages in rep["notBool"].values())
    assert rep["planar"] == {"renderPiece": mix.LOUDNESS_PLANAR, "renderScore": mix.LOUDNESS_PLANAR}
    assert set(rep["pcm"]) == calls - set(rep["planar"])
    for call, messages in rep["pcm"].items():
        assert messages == [mix.LOUDNESS_NOT_NUMBER] * 2 + [mix.TRUE_PEAK_MAX_BAD] * 2 + [mix.LOUDNESS_WITH_NORMALISE % 2], call
    d.configure(sv.SAMPLE_RATE)
    voices = lambda: [sv.voice(k) for k in range(3)]
    with_tracks = dict(tracks=[mc.clip, None], track_of=[0, 1, -1], faders=[1, 0.5], buses=[mc.comb], track_sends=[[1, 0]])
    empty = d.render_score(voices(), [0, 1, 2], 0.01, 0, stems=True, true_peak=True, **with_tracks)
    assert rep["empty"] == dict(plain(empty.meters), stems=empty.names, level=True)
    one = d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 0, loudness=-16)
    assert rep["one"] == dict(plain(one.meters), keys=["gain", "level", "meters", "mix"], gain=one.gain, level=float(one.level), bytes=one.mix.data.size)
    stems = d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 16, 0, stems=True, loudness=-23, true_peak_max=-2, **with_tracks)
    assert rep["stems"] == dict(names=stems.names, gain=stems.gain, level=float(stems.level), bytes=stems.mix.data.size, meters=stems.meters.names)
    assert rep["off"] is True and rep["none"] == [[0.0, 0.0]]  # (one signal of two channels)


@pytest.mark.gpu
def test_loudness_through_node_is_pythons(tmp_path):
    n, rate = 7, sv.SAMPLE_RATE
    d.configure(rate)
    onsets, _, gains = sv.layout(n)
    voice_duration, dur = (sv.NV + 0.5) / rate, (5 * 4800 + 17 + 0.5) / rate  # (two blocks and a last short hop)
    of2, f2, levels, pans = tc.track_of(n, 2), tc.faders(2), tc.levels(1, 2), pans_for(n)
    voices = lambda: [sv.voice(k) for k in range(n)]
    kw = dict(pans=pans, tracks=[mc.clip, None], track_of=of2, faders=f2, buses=[mc.comb], track_sends=levels, stems=True)
    host, host_rate = (0.3 * np.random.default_rng(2).standard_normal((3, 2, 1001))).astype(np.float32), 44100
    host[2, 1, 500] = np.inf
    spec = str(tmp_path / "loudness.json")
    host.tofile(spec[:-5] + ".host.f32")
    floats = lambda a: [float(x) for x in a]
    with open(spec, "w") as f:
        json.dump({"n": n, "onsets": onsets.tolist(), "gains": floats(gains), "voiceDuration": voice_duration, "duration": dur, "trackOf": of2.tolist(), "faders": floats(f2),
                   "trackSends": [floats(row) for row in levels], "pans": floats(pans), "hostRate": host_rate}, f)
    rep = node("render", spec)
    planar = d.render_piece(voices(), onsets, voice_duration, dur, None, gains, true_peak=True, **kw)
    assert rep["planar"] == dict(plain(planar.meters), stems=planar.names, level=True) and all(v > 0 for v in planar.meters.true_peak["mix"])
    pcm = d.render_piece_pcm(voices(), onsets, voice_duration, dur, 16, 0, None, gains, loudness=-23, **kw)
    assert rep["pcm"] == dict(plain(pcm.meters), gain=pcm.gain, level=float(pcm.level), frames=[sha(pcm[k].data) for k in pcm.names], peaks=[num(pcm.peaks[k]) for k in pcm.names])
    assert pcm.gain != 1.0 and rep["pcm"]["truePeak"] == rep["planar"]["truePeak"]
    limited = d.render_piece_pcm(voices(), onsets, voice_duration, dur, 24, 0, None, gains, loudness=0, true_peak_max=-1, **kw)
    assert rep["limited"] == dict(gain=limited.gain, level=float(limited.level), frames=[sha(limited[k].data) for k in limited.names]) and limited.gain != pcm.gain
    lone = d.render_piece_pcm(voices(), onsets, voice_duration, dur, 24, 0, None, gains, loudness=-16, true_peak_max=-2, **dict(kw, stems=False))
    assert rep["lone"] == dict(plain(lone.meters), keys=["gain", "level", "meters", "mix"], gain=lone.gain, level=float(lone.level), frames=sha(lone.mix.data), peak=num(lone.mix.peak))
    files = d.render_piece_wav(voices(), onsets, voice_duration, dur, 16, 0, None, gains, loudness=-23, **kw)
    assert rep["files"] == dict(gain=files.gain, level=float(files.level), files=[sha(files[k]) for k in files.names])
    want = render.true_peak(host, host_rate)
    assert rep["host"] == [[num(v) for v in row] for row in want] and rep["host"][2][1] == "NaN" and rep["hostOne"] == [[num(v) for v in want[0]]]
    assert np.array_equal(np.isnan(want), np.isnan(mix.true_peak(host, host_rate)))
