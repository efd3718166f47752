"""The `fracs` option of the JavaScript host on the GPU: renderPiece with fracs of a 13-voice panned list of two instruments equals what
Python's render_piece wrote to a file, bit for bit, and the oracle's render of the piece as ONE circuit whose Delay units take onset +
fraction, which is committed as tests/golden/frac_piece_13.pcm.f32 (tests/js/check_frac.js).  The refusal strings, which need no
device, are compared in tests/test_frac_host.py."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import score_voices as sv
from conftest import GOLDEN, ROOT
from dusp_amd import descriptor
from frac_cases import as_one_frac_circuit, layout, pans_for
from test_piece_host import NV_SAW, bits, interleaved_voice

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")
GOLDEN_PIECE = os.path.join(GOLDEN, "frac_piece_13.pcm.f32")
N = 13


def test_the_golden_fractional_piece_is_the_oracles_one_circuit(oracle):
    """planar f32 [2][sv.NT]: 13 voices of the interleaved list, frac_cases.layout's onsets, fractions and gains, pan_cases.pans_for's pans"""
    d.configure(sv.SAMPLE_RATE)
    onsets, fracs, gains = layout(N, True)
    circuit = as_one_frac_circuit([interleaved_voice(k) for k in range(N)], onsets, fracs, gains, pans_for(N))
    want = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
    golden = np.fromfile(GOLDEN_PIECE, dtype=np.float32).reshape(2, sv.NT)
    assert np.array_equal(bits(golden), bits(want))


@pytest.mark.gpu
def test_render_piece_with_fracs_through_node_is_pythons_and_the_oracles(tmp_path):
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    rate = sv.SAMPLE_RATE
    d.configure(rate)
    onsets, fracs, gains = layout(N, True)
    pans = pans_for(N)
    durations = [((sv.NV if k % 2 == 0 else NV_SAW) + 0.5) / rate for k in range(N)]
    dur = (sv.NT + 0.5) / rate
    piece = np.stack(d.render_piece([interleaved_voice(k) for k in range(N)], onsets, durations, dur, None, gains, pans=pans, fracs=fracs))
    assert piece.shape == (2, sv.NT) and np.abs(piece).max() > 0
    spec = str(tmp_path / "frac_piece.json")
    piece.astype(np.float32).tofile(spec[:-5] + ".f32")
    with open(spec, "w") as f:
        json.dump({"n": N, "sampleRate": rate, "nTotal": sv.NT, "onsets": onsets.tolist(), "fracs": fracs.tolist(), "gains": [float(g) for g in gains],
                   "pans": [float(p) for p in pans], "voiceDurations": durations, "duration": dur, "peak": float(np.abs(piece).max()), "golden": GOLDEN_PIECE}, f)
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_frac.js"), "--sampleRate=48000", "render", spec], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    assert rep["checked"] >= 14 and not rep["failed"], rep["failed"]
