"""Meters in the JavaScript host (dusp_amd/js): the refusal strings, the block count and what a call over no samples resolves to are
Python's — compared without a device — and, on the GPU, the doubles of renderPiece / renderPiecePcm / renderScore with meters and of
meter() are the doubles Python's calls return: both hosts hand on what the library computed (tests/js/check_meters.js)."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import meter_cases as mtc
import score_voices as sv
import track_cases as tc
from conftest import ROOT
from dusp_amd import mix, render
from pan_cases import pans_for
from test_piece_host import NV_SAW, interleaved_voice

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")


def node(*args):
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_meters.js"), "--sampleRate=48000"] + list(args), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
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
    """a render.Meters as tests/js/check_meters.js writes one"""
    return {"names": meters.names, "hop": meters.hop, "block": meters.block, "lufs": [num(meters.lufs[k]) for k in meters.names],
            "rms": [[num(v) for v in meters.rms[k]] for k in meters.names], "momentary": [[num(v) for v in meters.momentary[k]] for k in meters.names]}


def test_the_refusals_the_blocks_and_the_empty_meters_are_pythons():
    rep = node("surface")
    assert set(rep["refused"]) == {"renderPiece", "renderScore", "renderPiecePcm", "renderScorePcm", "renderPieceWav", "renderScoreWav"}
    for call, messages in rep["refused"].items():
        assert messages == [mix.METERS_NOT_BOOL] * 3 + [mix.STEMS_NOT_BOOL], call
    assert rep["rateLow"] == [mix.METER_RATE_LOW % 7999] * 2
    assert rep["blocks"] == [mix.meter_blocks(n, rate) for n, rate in ((3199, 8000), (3200, 8000), (3999, 8000), (4000, 8000), (32123, 8000), (44100, 11025), (88200, 44100),
                                                                       (19200, 48000), (1000000, 192000))]
    assert rep["hops"] == [mix.meter_hop(rate) for rate in (8000, 11025, 44100, 48000, 192000)]
    d.configure(sv.SAMPLE_RATE)
    voices = lambda: [sv.voice(k) for k in range(3)]
    with_tracks = dict(tracks=[mc.echo, None], track_of=[0, 1, -1], faders=[1, 0.5], buses=[mc.comb], track_sends=[[1, 0]])
    empty = d.render_score(voices(), [0, 1, 2], 0.01, 0, stems=True, meters=True, **with_tracks)
    assert rep["empty"] == dict(plain(empty.meters), stems=empty.names, mix=len(empty.mix))
    one = d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 2, meters=True)
    assert rep["one"] == dict(plain(one.meters), keys=["meters", "mix"], bytes=one.mix.data.size, bitDepth=one.mix.bitDepth)
    assert rep["off"] is True
    assert rep["none"] == plain(render.Meters(["0"], render._empty_meters(1, 2, 8000)))


@pytest.mark.gpu
def test_meters_through_node_are_pythons(tmp_path):
    n, rate = 13, sv.SAMPLE_RATE
    d.configure(rate)
    onsets, _, gains = sv.layout(n)
    durations = [((sv.NV if k % 2 == 0 else NV_SAW) + 0.5) / rate for k in range(n)]
    dur = (5 * 4800 + 17 + 0.5) / rate  # (two blocks and a last short hop)
    of3, f3, levels, pans = tc.track_of(n, 3), tc.faders(3), tc.levels(2, 3), pans_for(n)
    voices = lambda: [interleaved_voice(k) for k in range(n)]
    mono = lambda: [sv.voice(k) for k in range(n)]
    tracked = dict(tracks=[mc.clip, None, mc.echo], track_of=of3, faders=f3, buses=[mc.echo, mc.comb], track_sends=levels, stems=True, meters=True)
    host, host_rate = mtc.dc_noise(3 * 3200 + 17, (3, 2)), 8000
    host[2, 1, 5000] = np.inf
    spec = str(tmp_path / "meters.json")
    host.tofile(spec[:-5] + ".host.f32")
    floats = lambda a: [float(x) for x in a]
    with open(spec, "w") as f:
        json.dump({"n": n, "sampleRate": rate, "onsets": onsets.tolist(), "gains": floats(gains), "voiceDurations": durations, "duration": dur, "trackOf3": of3.tolist(),
                   "faders3": floats(f3), "trackSends": [floats(row) for row in levels], "pans": floats(pans), "hostRate": host_rate}, f)
    rep = node("render", spec)
    full = d.render_piece(voices(), onsets, durations, dur, None, gains, **tracked)
    assert rep["fullStems"] == full.names and rep["full"] == plain(full.meters)
    assert all(math.isfinite(full.meters.lufs[k]) for k in ("direct", "mix")) and full.meters.momentary["mix"].shape == (2,)
    assert rep["pcm"] == plain(d.render_piece_pcm(voices(), onsets, durations, dur, 16, 2, None, gains, **tracked).meters) == rep["full"]
    lone = d.render_piece(voices(), onsets, durations, dur, None, gains, master=mc.comb, meters=True)
    assert rep["lone"] == dict(plain(lone.meters), channels=1, samples=5 * 4800 + 17) and rep["loneIsTheMix"] is True
    assert rep["file"] == dict(plain(lone.meters), riff="RIFF") and rep["files"] == dict(plain(full.meters), riff="RIFFRIFF")
    assert rep["score"] == plain(d.render_score(mono(), onsets, durations[0], dur, None, gains, pans=pans, meters=True).meters)
    assert rep["host"] == plain(render.meter(host, host_rate)) and rep["host"]["lufs"][2] == "NaN" and rep["host"]["names"] == ["0", "1", "2"]
    assert rep["hostOne"] == plain(render.meter(host[0], host_rate))
