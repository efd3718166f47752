"""renderPiece / renderPiecePcm / renderPieceWav of the JavaScript host (dusp_amd/js): the grouping of a mixed voice list into parts, the
channel check and the refusal strings are twins of Python's — compared without a device — and, on the GPU, renderPiece of a 13-voice
list of two instruments equals what Python's render_piece wrote to a file, bit for bit (tests/js/check_piece.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import mix_voices
import score_voices as sv
from conftest import ROOT
from dusp_amd import descriptor, render
from test_piece_host import NV_SAW, interleaved_voice

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")


def node(*args):
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_piece.js"), "--sampleRate=48000"] + list(args), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    return rep


def test_the_grouping_and_the_refusals_are_pythons():
    rep = node("grouping")
    d.configure(sv.SAMPLE_RATE)
    kinds = ["score", "filtered_saw", "score", "pan", "filtered_saw", "score", "filtered_saw", "score"]
    samples = [773, 1031, 773, 500, 1031, 400, 1031, 773]
    made, voices = {}, []
    for kind in kinds:
        k = made.get(kind, 0)
        made[kind] = k + 1
        voices.append(sv.voice(k) if kind == "score" else mix_voices.voice(kind, k))
    grouped = render.piece_parts([descriptor.extract(v) for v in voices], samples)
    assert rep["partOf"] == grouped.part_of.tolist() == [0, 1, 0, 2, 1, 3, 1, 0] and rep["instanceOf"] == grouped.instance_of.tolist() and rep["sampleRate"] == grouped.sample_rate
    assert rep["parts"] == [[uni.n_instances, n, uni.n_params] for uni, n in grouped.parts]
    for p, (uni, _) in enumerate(grouped.parts):  # the same programs, word for word, and the same parameter tables
        words = np.array([np.nan if w == "nan" else w for w in rep["words"][p]], dtype=np.float64)
        assert np.array_equal(words, uni.words, equal_nan=True), p
        assert (rep["params"][p] is None) == (uni.params is None)
        assert uni.params is None or np.array_equal(np.array(rep["params"][p], dtype=np.float32), uni.params.reshape(-1)), p
    assert rep["keysAlike"] and rep["keysApart"] and rep["channels"] == [1, 2]
    r = rep["refusals"]
    want = "dusp-hip: the voices of a piece must have one number of output channels: part 1 has 2, part 0 has 1"
    assert r["channels"] == r["channelsPcm"] == r["channelsWav"] == r["check"] == want  # (Python's string: tests/test_piece_host.py)
    with pytest.raises(descriptor.DuspError) as e:
        render.check_piece_channels([1, 2, 1])
    assert str(e.value) == want
    assert r["none"] == "dusp-hip: no instances" and "whole numbers" in r["fraction"] and "voiceDurations must be one number or hold one value per outlet" in r["durations"]
    assert "lengths must lie in 0 .. the voice's own samples" in r["lengths"] and "voiceDuration must cover at least one sample" in r["noSample"]


@pytest.mark.gpu
def test_render_piece_through_node_is_pythons(tmp_path):
    n, rate = 13, sv.SAMPLE_RATE
    d.configure(rate)
    onsets, _, gains = sv.layout(n)
    samples = [sv.NV if k % 2 == 0 else NV_SAW for k in range(n)]
    lengths = [s - 7 * (k % 3) for k, s in enumerate(samples)]
    durations = [(s + 0.5) / rate for s in samples]
    dur = (sv.NT + 0.5) / rate
    piece = d.render_piece([interleaved_voice(k) for k in range(n)], onsets, durations, dur, lengths, gains)
    assert len(piece) == 1 and piece[0].shape == (sv.NT,) and np.abs(piece[0]).max() > 0
    spec = str(tmp_path / "piece.json")
    np.asarray(piece[0], dtype=np.float32).tofile(spec[:-5] + ".f32")
    with open(spec, "w") as f:
        json.dump({"n": n, "sampleRate": rate, "onsets": onsets.tolist(), "lengths": lengths, "gains": [float(g) for g in gains], "voiceDurations": durations, "duration": dur,
                   "peak": float(np.abs(piece[0]).max())}, f)
    rep = node("render", spec)
    assert rep["checked"] >= 6 and not rep["failed"], rep["failed"]
