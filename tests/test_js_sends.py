"""Effect sends in the JavaScript host (dusp_amd/js): the refusal strings and the table of levels are twins of Python's — compared
without a device — and, on the GPU, renderPiece / renderPiecePcm / renderScore with buses equal what Python's calls wrote to files, bit
for bit (tests/js/check_sends.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
import send_cases as sc
from conftest import ROOT
from dusp_amd import mix
from pan_cases import pans_for
from test_piece_host import NV_SAW, interleaved_voice
from test_sends_host import BUS_REFUSALS

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")


def node(*args):
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_sends.js"), "--sampleRate=48000"] + list(args), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    return rep


def test_the_refusals_and_the_table_of_levels_are_pythons():
    rep = node("surface")
    assert rep["table"] == mix.check_sends([[0, 0.5, 1], [1, 2, 3]], 3, 2).reshape(-1).tolist() and rep["oneBus"] == [0.25, 0.5, 1] and rep["noSamples"] == 0
    for case, (_, _, message) in BUS_REFUSALS.items():  # (tests/test_sends_host.py holds Python to the same strings)
        assert rep["bus"][case] == message, case
    s = rep["sends"]
    assert s["withoutBuses"] == s["score"] == s["piecePcm"] == s["scoreWav"] == mix.SENDS_WITHOUT_BUSES
    assert s["withoutSends"] == mix.BUSES_WITHOUT_SENDS
    assert (s["none"], s["five"], s["notAList"]) == (mix.BUS_COUNT % 0, mix.BUS_COUNT % 5, mix.BUS_COUNT % 0)
    assert s["fracs"] == s["places"] == s["stereo"] == mix.SENDS_PLACEMENT
    assert (s["short"], s["oneRowForTwo"]) == (mix.SENDS_SHAPE % (1, 3), mix.SENDS_SHAPE % (2, 3))
    assert (s["notFinite"], s["tooLarge"]) == (mix.SENDS_NOT_FINITE % (1, 0), mix.SENDS_NOT_FINITE % (2, 1))
    assert s["badBusInACall"] == mix.BUS_NOT_CALLABLE % 1


@pytest.mark.gpu
def test_buses_through_node_are_pythons(tmp_path):
    n, rate = 13, sv.SAMPLE_RATE
    d.configure(rate)
    onsets, _, gains = sv.layout(n)
    on5, _, g5 = sv.layout(5)
    durations = [((sv.NV if k % 2 == 0 else NV_SAW) + 0.5) / rate for k in range(n)]
    dur = (sv.NT + 0.5) / rate
    levels, five = sc.levels(n, 3), sc.levels(5)[0]
    voices = lambda: [interleaved_voice(k) for k in range(n)]
    mono = lambda: [sv.voice(k) for k in range(5)]
    piece = np.stack(d.render_piece(voices(), onsets, durations, dur, None, gains, buses=[mc.echo], sends=levels[0]))
    three = np.stack(d.render_piece(voices(), onsets, durations, dur, None, gains, buses=[mc.echo, mc.comb, mc.clip], sends=levels))
    master = np.stack(d.render_piece(voices(), onsets, durations, dur, None, gains, buses=[mc.echo, mc.clip], sends=levels[[0, 2]], master=mc.comb))
    pan = np.stack(d.render_piece(mono(), on5, durations[0], dur, None, g5, pans=pans_for(5), buses=[[mc.echo_of(300.25), mc.echo_of(411.5)]], sends=five))
    score = np.stack(d.render_score(mono(), on5, durations[0], dur, None, g5, buses=[mc.echo], sends=five))
    assert piece.shape == three.shape == master.shape == score.shape == (1, sv.NT) and pan.shape == (2, sv.NT) and np.abs(piece).max() > 0
    spec = str(tmp_path / "sends.json")
    for tag, a in (("", piece), (".three", three), (".master", master), (".pan", pan), (".score", score)):
        a.tofile(spec[:-5] + tag + ".f32")
    with open(spec, "w") as f:
        json.dump({"n": n, "sampleRate": rate, "onsets": onsets.tolist(), "gains": [float(g) for g in gains], "voiceDurations": durations, "duration": dur,
                   "sends": [[float(x) for x in row] for row in levels], "fiveOnsets": on5.tolist(), "fiveGains": [float(g) for g in g5], "fiveSends": [float(x) for x in five],
                   "pans": [float(p) for p in pans_for(5)], "peak": float(np.abs(piece).max())}, f)
    rep = node("render", spec)
    assert rep["checked"] >= 9 and not rep["failed"], rep["failed"]
