"""The `places` option of the JavaScript host on the GPU: renderPiece with places of a 13-voice list of two instruments equals the
contract (dusp_amd/mix.py score_chain_rows_placed) at the gains spaceTaps returned, what Python's render_piece wrote to a file — both
hosts' gains agree bit for bit for these places, which is asserted — and the oracle's channel-by-channel render of the anchor circuit,
which is committed as tests/golden/space_piece_13.pcm.f32 (tests/js/check_space.js).  The refusal strings, which need no device, are
compared in tests/test_space_host.py."""
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
from dusp_amd.mix import score_chain_rows_placed
from space_cases import SDPM, anchor_circuit, decibels, layout
from test_piece_host import NV_SAW, bits, interleaved_voice, oracle_rows

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")
GOLDEN_PIECE = os.path.join(GOLDEN, "space_piece_13.pcm.f32")
N = 13


def test_the_golden_placed_piece_is_the_oracles_anchor_channel_by_channel(oracle):
    """planar f32 [2][sv.NT]: 13 voices of the interleaved list, space_cases.layout's onsets, gains, places and stereo speakers"""
    d.configure(sv.SAMPLE_RATE)
    onsets, gains, places, speakers, delays, _ = layout(N, 2)
    db = decibels(places, speakers)
    golden = np.fromfile(GOLDEN_PIECE, dtype=np.float32).reshape(2, sv.NT)
    for c in range(2):
        circuit = anchor_circuit([interleaved_voice(k) for k in range(N)], onsets, db, delays, c, gains)
        want = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
        assert np.array_equal(bits(golden[c:c + 1]), bits(want)), c


@pytest.mark.gpu
def test_render_piece_with_places_through_node_is_the_contract_pythons_and_the_oracles(tmp_path, oracle):
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    rate = sv.SAMPLE_RATE
    d.configure(rate)
    onsets, gains, places, speakers, delays, tap_gains = layout(N, 2)
    durations = [((sv.NV if k % 2 == 0 else NV_SAW) + 0.5) / rate for k in range(N)]
    dur = (sv.NT + 0.5) / rate
    piece = np.stack(d.render_piece([interleaved_voice(k) for k in range(N)], onsets, durations, dur, None, gains, places=places, speakers=speakers, sample_delay_per_metre=SDPM))
    contract = score_chain_rows_placed(oracle_rows(N, oracle), onsets, delays, tap_gains, sv.NT, gains=gains)
    assert piece.shape == contract.shape == (2, sv.NT) and np.abs(piece).max() > 0
    spec = str(tmp_path / "space_piece.json")
    contract.tofile(spec[:-5] + ".f32")
    piece.astype(np.float32).tofile(spec[:-5] + ".python.f32")
    with open(spec, "w") as f:
        json.dump({"n": N, "sampleRate": rate, "nTotal": sv.NT, "onsets": onsets.tolist(), "voiceGains": [float(g) for g in gains], "places": [[float(x) for x in p] for p in places],
                   "speakers": speakers, "sampleDelayPerMetre": SDPM, "delays": delays.ravel().tolist(), "gains": tap_gains.ravel().tolist(), "voiceDurations": durations,
                   "duration": dur, "peak": float(np.abs(piece).max()), "golden": GOLDEN_PIECE}, f)
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_space.js"), "--sampleRate=48000", "render", spec], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    assert rep["checked"] >= 16 and not rep["failed"], rep["failed"]
