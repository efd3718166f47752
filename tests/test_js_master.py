"""The master of a score or piece in the JavaScript host (dusp_amd/js): the refusal strings and the unified master's parameter table are
twins of Python's — compared without a device — and, on the GPU, renderPiece / renderPiecePcm / renderScore with a master equal what
Python's calls wrote to files, bit for bit (tests/js/check_master.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
import stereo_cases as sc
from conftest import ROOT
from dusp_amd import mix
from test_master_host import REFUSALS
from test_piece_host import NV_SAW, interleaved_voice

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")


def node(*args):
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_master.js"), "--sampleRate=48000"] + list(args), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    return rep


def test_the_refusals_and_the_parameter_table_are_pythons():
    rep = node("surface")
    uni = mc.unified_master([mc.echo_of(300.25), mc.echo_of(411.5)], 2)
    two = rep["two"]
    assert (two["nParams"], two["nInstances"], two["params"]) == (uni.n_params, uni.n_instances, uni.params.reshape(-1).tolist()) == (1, 2, [300.25, 411.5])
    assert np.array_equal(np.array([np.nan if w == "nan" else w for w in two["words"]], dtype=np.float64), uni.words, equal_nan=True)  # the same program, word for word
    assert rep["one"] == {"nParams": 0, "nInstances": 3} and rep["noSamples"] == 0
    r = rep["refusals"]
    for case, (_, _, message) in REFUSALS.items():  # (tests/test_master_host.py holds Python to the same strings)
        assert r[case] == message, case
    assert r["inputAlone"] == mix.MASTER_INPUT_ALONE
    assert r["piece"] == r["score"] == r["piecePcm"] == r["scoreWav"] == mix.MASTER_NOT_CALLABLE


@pytest.mark.gpu
def test_a_master_through_node_is_pythons(tmp_path):
    n, rate = 13, sv.SAMPLE_RATE
    d.configure(rate)
    onsets, _, gains = sv.layout(n)
    on5, _, g5 = sv.layout(5)
    durations = [((sv.NV if k % 2 == 0 else NV_SAW) + 0.5) / rate for k in range(n)]
    dur = (sv.NT + 0.5) / rate
    piece = np.stack(d.render_piece([interleaved_voice(k) for k in range(n)], onsets, durations, dur, None, gains, master=mc.echo))
    stereo = np.stack(d.render_piece([sc.voice(k, sc.TWO) for k in range(5)], on5, durations[0], dur, None, g5, master=[mc.echo_of(300.25), mc.echo_of(411.5)]))
    score = np.stack(d.render_score([sv.voice(k) for k in range(5)], on5, durations[0], dur, None, g5, master=mc.echo))
    assert piece.shape == (1, sv.NT) and stereo.shape == (2, sv.NT) and score.shape == (1, sv.NT) and np.abs(piece).max() > 0
    spec = str(tmp_path / "master.json")
    piece.tofile(spec[:-5] + ".f32")
    stereo.tofile(spec[:-5] + ".stereo.f32")
    score.tofile(spec[:-5] + ".score.f32")
    with open(spec, "w") as f:
        json.dump({"n": n, "sampleRate": rate, "onsets": onsets.tolist(), "gains": [float(g) for g in gains], "voiceDurations": durations, "duration": dur,
                   "stereoOnsets": on5.tolist(), "stereoGains": [float(g) for g in g5], "peak": float(np.abs(piece).max())}, f)
    rep = node("render", spec)
    assert rep["checked"] >= 7 and not rep["failed"], rep["failed"]
