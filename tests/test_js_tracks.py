"""Tracks in the JavaScript host (dusp_amd/js): the refusal strings, checkTracks' arrays and trackPrograms' groups are twins of Python's
— compared without a device — and, on the GPU, renderPiece / renderPiecePcm / renderScore with tracks equal what Python's calls wrote to
files, bit for bit (tests/js/check_tracks.js)."""
import json
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
from frac_cases import layout as frac_layout
from pan_cases import pans_for
from test_piece_host import NV_SAW, interleaved_voice
from test_tracks_host import TRACK_REFUSALS

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")


def node(*args):
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_tracks.js"), "--sampleRate=48000"] + list(args), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    return rep


def test_the_refusals_the_arrays_and_the_groups_are_pythons():
    rep = node("surface")
    of, f, s = mix.check_tracks(3, 2, [0, -1, 1], [0.5, 2], [[0, 1], [1, 0.25]], 2)
    assert rep["trackOf"] == of.tolist() and rep["faders"] == f.tolist() and rep["trackSends"] == s.reshape(-1).tolist() and rep["oneBus"] == [0.5, 1]
    assert rep["none"] == {"trackOf": None, "faders": None, "trackSends": None} and rep["noSamples"] == [0, 0, 0]
    d.configure(sv.SAMPLE_RATE)
    groups = render.track_programs([mc.echo_of(300.25), mc.clip, None, mc.echo_of(411.5), [mc.echo_of(100.5)], mc.clip], 1, sv.SAMPLE_RATE)
    assert rep["groups"] == [{"tracks": which, "nInstances": uni.n_instances, "params": uni.params.reshape(-1).tolist() if uni.n_params else []} for uni, which in groups]
    wide = render.track_programs([[mc.echo_of(300.25), mc.echo_of(411.5)], mc.echo_of(100.5)], 2, sv.SAMPLE_RATE)
    assert rep["wide"] == [{"tracks": which, "nInstances": uni.n_instances, "params": uni.params.reshape(-1).tolist()} for uni, which in wide]
    for case, (_, _, message) in TRACK_REFUSALS.items():  # (tests/test_tracks_host.py holds Python to the same strings)
        assert rep["track"][case] == message, case
    t = rep["tracks"]
    assert t["trackOfAlone"] == t["score"] == t["piecePcm"] == t["scoreWav"] == mix.TRACKS_TRACK_OF_ALONE
    assert (t["fadersAlone"], t["sendsAlone"]) == (mix.TRACKS_NEED_TRACKS % "faders", mix.TRACKS_NEED_TRACKS % "track_sends")
    assert t["withoutTrackOf"] == mix.TRACKS_WITHOUT_TRACK_OF
    assert (t["none"], t["nine"], t["notAList"]) == (mix.TRACKS_COUNT % 0, mix.TRACKS_COUNT % 9, mix.TRACKS_COUNT % 0)
    assert t["short"] == t["notWhole"] == mix.TRACKS_TRACK_OF_SHAPE % 3
    assert (t["tooHigh"], t["tooLow"]) == (mix.TRACKS_TRACK_OF_RANGE % (1, 2, 2, 1), mix.TRACKS_TRACK_OF_RANGE % (2, -2, 2, 1))
    assert (t["fadersShape"], t["faderNaN"], t["faderTooLarge"]) == (mix.TRACKS_FADERS_SHAPE % 2, mix.TRACKS_FADER_NOT_FINITE % 1, mix.TRACKS_FADER_NOT_FINITE % 0)
    assert (t["sendsWithoutBuses"], t["busesWithoutSends"]) == (mix.TRACKS_SENDS_WITHOUT_BUSES, mix.TRACKS_BUSES_WITHOUT_SENDS)
    assert t["withSends"] == t["withBoth"] == mix.TRACKS_WITH_SENDS
    assert (t["noBuses"], t["fiveBuses"]) == (mix.BUS_COUNT % 0, mix.BUS_COUNT % 5)
    assert (t["sendsShape"], t["oneRowForTwo"]) == (mix.TRACKS_SENDS_SHAPE % (1, 2), mix.TRACKS_SENDS_SHAPE % (2, 2))
    assert t["levelNotFinite"] == mix.TRACKS_LEVEL_NOT_FINITE % (0, 1)
    assert t["badTrackInACall"] == mix.TRACK_NOT_CALLABLE % 1


@pytest.mark.gpu
def test_tracks_through_node_are_pythons(tmp_path):
    n, rate = 13, sv.SAMPLE_RATE
    d.configure(rate)
    onsets, _, gains = sv.layout(n)
    on5, fr5, g5 = frac_layout(5, True)
    durations = [((sv.NV if k % 2 == 0 else NV_SAW) + 0.5) / rate for k in range(n)]
    dur = (sv.NT + 0.5) / rate
    of2, of3, of5 = tc.track_of(n, 2), tc.track_of(n, 3), tc.track_of(5, 2)
    f2, f3, levels, lv5 = tc.faders(2), tc.faders(3), tc.levels(2, 3, 1), tc.levels(1, 2)
    voices = lambda: [interleaved_voice(k) for k in range(n)]
    mono = lambda: [sv.voice(k) for k in range(5)]
    piece = np.stack(d.render_piece(voices(), onsets, durations, dur, None, gains, tracks=[mc.clip, mc.echo], track_of=of2, faders=f2))
    three = np.stack(d.render_piece(voices(), onsets, durations, dur, None, gains, tracks=[mc.echo_of(300.25), mc.echo_of(411.5), mc.echo_of(257.75)], track_of=of3))
    full = np.stack(d.render_piece(voices(), onsets, durations, dur, None, gains, tracks=[mc.clip, None, mc.echo], track_of=of3, faders=f3, buses=[mc.echo, mc.comb],
                                   track_sends=levels, master=mc.comb))
    pan = np.stack(d.render_piece(mono(), on5, durations[0], dur, None, g5, pans=pans_for(5), fracs=fr5, tracks=[[mc.echo_of(300.25), mc.echo_of(411.5)], None], track_of=of5,
                                  faders=f2, buses=[mc.clip], track_sends=lv5))
    score = np.stack(d.render_score(mono(), on5, durations[0], dur, None, g5, tracks=[mc.echo, mc.comb], track_of=of5, faders=f2))
    assert piece.shape == three.shape == full.shape == score.shape == (1, sv.NT) and pan.shape == (2, sv.NT) and np.abs(piece).max() > 0
    spec = str(tmp_path / "tracks.json")
    for tag, a in (("", piece), (".three", three), (".full", full), (".pan", pan), (".score", score)):
        a.tofile(spec[:-5] + tag + ".f32")
    floats = lambda a: [float(x) for x in a]
    with open(spec, "w") as f:
        json.dump({"n": n, "sampleRate": rate, "onsets": onsets.tolist(), "gains": floats(gains), "voiceDurations": durations, "duration": dur,
                   "trackOf2": of2.tolist(), "trackOf3": of3.tolist(), "faders2": floats(f2), "faders3": floats(f3), "trackSends": [floats(row) for row in levels],
                   "fiveOnsets": on5.tolist(), "fiveFracs": floats(fr5), "fiveGains": floats(g5), "fiveTrackOf": of5.tolist(), "fiveLevels": floats(lv5[0]),
                   "pans": floats(pans_for(5)), "peak": float(np.abs(piece).max())}, f)
    rep = node("render", spec)
    assert rep["checked"] >= 9 and not rep["failed"], rep["failed"]
