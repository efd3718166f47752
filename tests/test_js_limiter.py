"""The limiter of a loudness delivery in the JavaScript host (dusp_amd/js): the refusal strings, the window in samples and what a call
over no samples resolves to are Python's — compared without a device — and, on the GPU, the limiter's record, the meters, the gain,
the level and the frames of renderPiecePcm / renderPieceWav with limiter: true, and what limit() returns, are what Python's calls
return: both hosts hand on what the library computed (tests/js/check_limiter.js)."""
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
from dusp_amd import mix, render
from pan_cases import pans_for

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")


def node(*args):
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_limiter.js"), "--sampleRate=48000"] + list(args), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
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
    return {"names": meters.names, "lufs": [num(meters.lufs[k]) for k in meters.names], "rms": [[num(v) for v in meters.rms[k]] for k in meters.names],
            "truePeak": [[num(v) for v in meters.true_peak[k]] for k in meters.names]}


def record(lim):
    """a render.Limiter as tests/js/check_limiter.js writes one"""
    return {"engaged": lim.engaged, "threshold": num(lim.threshold), "window": lim.window, "reduction": num(lim.reduction), "lufsIn": num(lim.lufs_in), "truePeakIn": num(lim.true_peak_in)}


def sha(data):
    return hashlib.sha256(data if isinstance(data, bytes) else np.ascontiguousarray(data).tobytes()).hexdigest()


def test_the_refusals_the_windows_and_the_empty_results_are_pythons():
    rep = node("surface")
    calls = {"renderPiece", "renderScore", "renderPiecePcm", "renderScorePcm", "renderPieceWav", "renderScoreWav"}
    assert set(rep["notBool"]) == calls and all(messages == [mix.LIMITER_NOT_BOOL] * 2 + [mix.TRUE_PEAK_NOT_BOOL] for messages in rep["notBool"].values())
    assert rep["planar"] == {name: [mix.LIMITER_NEEDS_LOUDNESS, mix.LOUDNESS_PLANAR] for name in ("renderPiece", "renderScore")}
    assert set(rep["pcm"]) == calls - set(rep["planar"])
    for call, messages in rep["pcm"].items():
        assert messages == [mix.LIMITER_NEEDS_LOUDNESS] + [mix.LIMITER_WINDOW_BAD] * 3 + [mix.LIMITER_WINDOW_LONG % (48000, 48000), mix.LIMITER_WINDOW_LONG % (2 ** 62, 48000), mix.LIMITER_WINDOW_LONG % (int(12345.678 * 48000), 48000),
                            mix.LOUDNESS_WITH_NORMALISE % 2], call
    d.configure(sv.SAMPLE_RATE)
    assert sv.SAMPLE_RATE == 48000
    voices = lambda: [sv.voice(k) for k in range(3)]
    with_tracks = dict(tracks=[mc.clip, None], track_of=[0, 1, -1], faders=[1, 0.5], buses=[mc.comb], track_sends=[[1, 0]])
    one = d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 0, loudness=-16, limiter=True)
    assert rep["one"] == dict(keys=["gain", "level", "limiter", "meters", "mix"], gain=one.gain, limiter=record(one.limiter)) and one.limiter.window == 240
    files = d.render_score_pcm(voices(), [0, 1, 2], 0.01, 0, 16, 0, stems=True, loudness=-23, limiter=True, limiter_window=0.001, **with_tracks)
    assert rep["files"] == dict(names=files.names, limiter=record(files.limiter)) and files.limiter.window == 48
    assert rep["off"] is True
    # the window in samples: Python's round, halves to the even number
    assert rep["windows"] == [mix.check_limiter(True, w, -16, rate) for w, rate in ((0.005, 48000), (0.005, 44100), (0.005, 8000), (1e-9, 8000), (4096 / 48000, 48000), (0.0025, 1000), (0.0035, 1000))]
    assert rep["windows"] == [240, 220, 40, 1, 4096, 2, 4]
    assert rep["limit"] == [mix.LIMITER_THRESHOLD_BAD] * 2 + [mix.LIMITER_WINDOW_SAMPLES] * 3 and rep["none"] == [2, 0, 1]


@pytest.mark.gpu
def test_the_limiter_through_node_is_pythons(tmp_path):
    n, rate = 7, sv.SAMPLE_RATE
    d.configure(rate)
    onsets, _, gains = sv.layout(n)
    voice_duration, dur = (sv.NV + 0.5) / rate, (5 * 4800 + 17 + 0.5) / rate  # (two blocks and a last short hop)
    of2, f2, levels, pans = tc.track_of(n, 2), tc.faders(2), tc.levels(1, 2), pans_for(n)
    voices = lambda: [sv.voice(k) for k in range(n)]
    kw = dict(pans=pans, tracks=[mc.clip, None], track_of=of2, faders=f2, buses=[mc.comb], track_sends=levels, stems=True)
    # the targets: 6 dB above and below the one at which the largest true peak meets the ceiling of -1 dBTP
    base = d.render_piece(voices(), onsets, voice_duration, dur, None, gains, true_peak=True, **kw)
    meets = base.meters.lufs["mix"] + 20 * math.log10(10 ** (-1 / 20) / max(v.max() for v in base.meters.true_peak.values()))
    high, low = meets + 6.0, meets - 6.0
    host, host_rate = (0.3 * np.random.default_rng(2).standard_normal((3, 2, 1001))).astype(np.float32), 44100
    host[2, 1, 500] = np.inf
    spec = str(tmp_path / "limiter.json")
    host.tofile(spec[:-5] + ".host.f32")
    floats = lambda a: [float(x) for x in a]
    with open(spec, "w") as f:
        json.dump({"n": n, "onsets": onsets.tolist(), "gains": floats(gains), "voiceDuration": voice_duration, "duration": dur, "trackOf": of2.tolist(), "faders": floats(f2),
                   "trackSends": [floats(row) for row in levels], "pans": floats(pans), "hostRate": host_rate, "high": high, "low": low, "threshold": 0.4, "window": 33}, f)
    rep = node("render", spec)
    engaged = d.render_piece_pcm(voices(), onsets, voice_duration, dur, 24, 0, None, gains, loudness=high, true_peak_max=-1, limiter=True, **kw)
    assert engaged.limiter.engaged and engaged.limiter.window == 240 and engaged.limiter.reduction < 1.0
    assert rep["engaged"] == dict(plain(engaged.meters), gain=engaged.gain, level=float(engaged.level), limiter=record(engaged.limiter), frames=[sha(engaged[k].data) for k in engaged.names],
                                  peaks=[num(engaged.peaks[k]) for k in engaged.names])
    idle = d.render_piece_pcm(voices(), onsets, voice_duration, dur, 16, 0, None, gains, loudness=low, limiter=True, limiter_window=0.01, **kw)
    assert not idle.limiter.engaged and idle.limiter.window == 480
    assert rep["idle"] == dict(plain(idle.meters), gain=idle.gain, level=float(idle.level), limiter=record(idle.limiter), frames=[sha(idle[k].data) for k in idle.names])
    lone = d.render_piece_pcm(voices(), onsets, voice_duration, dur, 16, 0, None, gains, loudness=high, true_peak_max=-2, limiter=True, limiter_window=0.002, **dict(kw, stems=False))
    assert rep["lone"] == dict(plain(lone.meters), keys=["gain", "level", "limiter", "meters", "mix"], gain=lone.gain, level=float(lone.level), limiter=record(lone.limiter), frames=sha(lone.mix.data),
                               peak=num(lone.mix.peak)) and lone.limiter.engaged and lone.limiter.window == 96
    files = d.render_piece_wav(voices(), onsets, voice_duration, dur, 16, 0, None, gains, loudness=high, limiter=True, **kw)
    assert rep["files"] == dict(gain=files.gain, level=float(files.level), limiter=record(files.limiter), files=[sha(files[k]) for k in files.names])
    limited, g, reduction = render.limit(host, host_rate, 0.4, 33)
    assert rep["host"] == dict(data=sha(limited), gain=sha(g), reduction=reduction) and reduction < 1.0 and np.isinf(limited[2, 1, 500])
    alone = render.limit(host[0], host_rate, 0.4, 33)
    assert rep["hostOne"] == dict(data=sha(alone[0]), reduction=alone[2])
