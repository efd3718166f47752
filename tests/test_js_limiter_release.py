"""The limiter's release of its own in the JavaScript host (dusp_amd/js): the refusal strings, the release in samples and
what a call over no samples resolves to are Python's — compared without a device — and, on the GPU, the limiter's record, the meters, the
gain, the level and the frames of renderPiecePcm / renderPieceWav with limiter: true, limiterRelease, and what limit() returns with a
release, are what Python's calls return: both hosts hand on what the library computed (tests/js/check_limiter_release.js)."""
import json
import math
import os
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
from test_js_limiter import ADDON, NODE, num, plain, sha


def node(*args):
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_limiter_release.js"), "--sampleRate=48000"] + list(args), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    return rep


def record(lim):
    """a render.Limiter as tests/js/check_limiter_release.js writes one"""
    return {"engaged": lim.engaged, "threshold": num(lim.threshold), "window": lim.window, "reduction": num(lim.reduction), "lufsIn": num(lim.lufs_in), "truePeakIn": num(lim.true_peak_in),
            "release": lim.release}


def test_the_refusals_the_releases_and_the_empty_results_are_pythons():
    rep = node("surface")
    assert rep["planar"] == {name: [mix.LOUDNESS_PLANAR, mix.LIMITER_NEEDS_LOUDNESS, mix.LIMITER_RELEASE_NEEDS_LIMITER] for name in ("renderPiece", "renderScore")}
    assert set(rep["pcm"]) == {"renderPiecePcm", "renderScorePcm", "renderPieceWav", "renderScoreWav"}
    for call, messages in rep["pcm"].items():
        assert messages == [mix.LIMITER_RELEASE_NEEDS_LIMITER] * 2 + [mix.LIMITER_RELEASE_BAD] * 4 + [mix.LIMITER_RELEASE_LONG % (48000000, 48000), mix.LIMITER_RELEASE_LONG % (2 ** 62, 48000),
                                                                                                    mix.LIMITER_WINDOW_LONG % (48000, 48000), mix.LIMITER_NEEDS_LOUDNESS], call
    d.configure(sv.SAMPLE_RATE)
    assert sv.SAMPLE_RATE == 48000
    voices = lambda: [sv.voice(k) for k in range(3)]
    one = d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 0, loudness=-16, limiter=True, limiter_release=0.05)
    assert rep["one"] == dict(keys=["gain", "level", "limiter", "meters", "mix"], gain=one.gain, limiter=record(one.limiter)) and one.limiter.release == 2400
    none = d.render_score_pcm(voices(), [0, 1, 2], 0.01, 0, 16, 0, loudness=-16, limiter=True)
    assert rep["none"] == record(none.limiter) and none.limiter.release == 0
    cases = ((0.05, 48000), (0.5, 44100), (1e-9, 8000), ((1 << 22) / 48000, 48000), (0.0025, 1000), (0.0035, 1000), (1, 8000))
    assert rep["releases"] == [mix.check_limiter_release(r, True, rate) for r, rate in cases] == [2400, 22050, 1, 1 << 22, 2, 4, 8000] and rep["absent"] == [0, 0]
    assert rep["limit"] == [mix.LIMITER_RELEASE_SAMPLES] * 4 and rep["empty"] == [2, 0, 1]


@pytest.mark.gpu
def test_the_release_through_node_is_pythons(tmp_path):
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
    spec = str(tmp_path / "limiter_release.json")
    host.tofile(spec[:-5] + ".host.f32")
    floats = lambda a: [float(x) for x in a]
    with open(spec, "w") as f:
        json.dump({"n": n, "onsets": onsets.tolist(), "gains": floats(gains), "voiceDuration": voice_duration, "duration": dur, "trackOf": of2.tolist(), "faders": floats(f2),
                   "trackSends": [floats(row) for row in levels], "pans": floats(pans), "hostRate": host_rate, "high": high, "low": low, "threshold": 0.4, "window": 33, "release": 700}, f)
    rep = node("render", spec)
    engaged = d.render_piece_pcm(voices(), onsets, voice_duration, dur, 24, 0, None, gains, loudness=high, true_peak_max=-1, limiter=True, limiter_release=0.05, **kw)
    assert engaged.limiter.engaged and engaged.limiter.window == 240 and engaged.limiter.release == 2400 and engaged.limiter.reduction < 1.0
    assert rep["engaged"] == dict(plain(engaged.meters), gain=engaged.gain, level=float(engaged.level), limiter=record(engaged.limiter), frames=[sha(engaged[k].data) for k in engaged.names],
                                  peaks=[num(engaged.peaks[k]) for k in engaged.names])
    without = d.render_piece_pcm(voices(), onsets, voice_duration, dur, 24, 0, None, gains, loudness=high, true_peak_max=-1, limiter=True, **kw)
    assert rep["engaged"]["frames"] != [sha(without[k].data) for k in without.names], "the release shows in the frames"
    idle = d.render_piece_pcm(voices(), onsets, voice_duration, dur, 16, 0, None, gains, loudness=low, limiter=True, limiter_window=0.01, limiter_release=0.5, **kw)
    assert not idle.limiter.engaged and idle.limiter.window == 480 and idle.limiter.release == 24000
    assert rep["idle"] == dict(plain(idle.meters), gain=idle.gain, level=float(idle.level), limiter=record(idle.limiter), frames=[sha(idle[k].data) for k in idle.names])
    files = d.render_piece_wav(voices(), onsets, voice_duration, dur, 16, 0, None, gains, loudness=high, limiter=True, limiter_release=0.2, **dict(kw, stems=False))
    assert rep["files"] == dict(gain=files.gain, level=float(files.level), limiter=record(files.limiter), file=sha(files.mix)) and files.limiter.release == 9600
    limited, g, reduction = render.limit(host, host_rate, 0.4, 33, 700)
    assert rep["host"] == dict(data=sha(limited), gain=sha(g), reduction=reduction) and reduction < 1.0
    plain_g = render.limit(host, host_rate, 0.4, 33)
    assert rep["hostPlain"] == dict(gain=sha(plain_g[1]), reduction=plain_g[2]) and rep["hostPlain"]["gain"] != rep["host"]["gain"]
