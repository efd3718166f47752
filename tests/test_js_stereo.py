"""The `stereo` option of the JavaScript host on the GPU: renderPiece of a 13-voice list of panned mono voices, plain mono voices and
voices of two channels in turn equals the contract (dusp_amd/mix.py score_chain_rows_stereo over the oracle's per-voice renders), what
Python's render_piece wrote to a file, bit for bit, and the oracle's render of the piece as ONE circuit, which is committed as
tests/golden/stereo_piece_13.pcm.f32 (tests/js/check_stereo.js).  The refusal strings, which need no device, are compared in
tests/test_stereo_host.py."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import score_voices as sv
import stereo_cases as sc
from conftest import GOLDEN, ROOT
from dusp_amd import descriptor
from dusp_amd.mix import score_chain_rows_stereo
from test_piece_host import bits

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")
GOLDEN_PIECE = os.path.join(GOLDEN, "stereo_piece_13.pcm.f32")
N, ORDER = 13, "in_turn"


def test_the_golden_stereo_piece_is_the_oracles_one_circuit(oracle):
    """planar f32 [2][sv.NT]: 13 voices, the kinds in turn, sv.layout's onsets and gains, stereo_cases.stereo_pans' pans"""
    d.configure(sv.SAMPLE_RATE)
    onsets, _, gains = sv.layout(N)
    circuit = sc.as_one_stereo_circuit(sc.voices_for(N, ORDER), onsets, sc.stereo_pans(N, ORDER), gains)
    want = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
    golden = np.fromfile(GOLDEN_PIECE, dtype=np.float32).reshape(2, sv.NT)
    assert np.array_equal(bits(golden), bits(want))


@pytest.mark.gpu
def test_render_piece_stereo_through_node_is_the_contract_pythons_and_the_oracles(tmp_path, oracle):
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    rate = sv.SAMPLE_RATE
    d.configure(rate)
    onsets, _, gains = sv.layout(N)
    pans = sc.stereo_pans(N, ORDER)
    voice_dur, dur = (sv.NV + 0.5) / rate, (sv.NT + 0.5) / rate
    piece = np.stack(d.render_piece(sc.voices_for(N, ORDER), onsets, voice_dur, dur, None, gains, pans=pans, stereo=True))
    assert piece.shape == (2, sv.NT) and np.abs(piece).max() > 0
    # the contract over the oracle's renders voice by voice
    rows = [np.asarray(oracle.render(descriptor.extract(v).words, sv.NV), dtype=np.float32) for v in sc.voices_for(N, ORDER)]
    assert [r.shape for r in rows] == [(2 if kind == sc.TWO else 1, sv.NV) for kind in sc.kinds_for(N, ORDER)]
    contract = score_chain_rows_stereo(rows, onsets, pans, sv.NT, None, gains)
    assert np.array_equal(bits(piece), bits(contract))
    frac_onsets, fracs, _ = sc.layout(N, True)
    with_fracs = np.stack(d.render_piece(sc.voices_for(N, ORDER), frac_onsets, voice_dur, dur, None, gains, pans=pans, fracs=fracs, stereo=True))
    assert np.array_equal(bits(with_fracs), bits(score_chain_rows_stereo(rows, frac_onsets, pans, sv.NT, None, gains, fracs=fracs)))
    spec = str(tmp_path / "stereo_piece.json")
    piece.astype(np.float32).tofile(spec[:-5] + ".f32")
    with_fracs.astype(np.float32).tofile(spec[:-5] + ".frac.f32")
    contract.astype(np.float32).tofile(spec[:-5] + ".contract.f32")
    with open(spec, "w") as f:
        json.dump({"n": N, "sampleRate": rate, "nTotal": sv.NT, "onsets": onsets.tolist(), "gains": [float(g) for g in gains],
                   "pans": [None if np.isnan(p) else float(p) for p in pans], "voiceDuration": voice_dur, "duration": dur, "peak": float(np.abs(piece).max()),
                   "fracOnsets": frac_onsets.tolist(), "fracs": fracs.tolist(), "golden": GOLDEN_PIECE, "contract": spec[:-5] + ".contract.f32"}, f)
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_stereo.js"), "--sampleRate=48000", "render", spec], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    assert rep["checked"] >= 17 and not rep["failed"], rep["failed"]
