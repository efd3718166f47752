"""Stems in the JavaScript host (dusp_amd/js): the refusal string, the names and what a call over no samples resolves to are Python's —
compared without a device — and, on the GPU, renderPiece / renderPiecePcm / renderPieceWav / renderScore with stems equal what Python's
calls wrote to files, bit for bit (tests/js/check_stems.js)."""
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
import stem_cases as stc
import track_cases as tc
from conftest import ROOT
from dusp_amd import mix, wav
from pan_cases import pans_for
from test_piece_host import NV_SAW, interleaved_voice

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")


def node(*args):
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_stems.js"), "--sampleRate=48000"] + list(args), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    return rep


def test_the_refusal_the_names_and_the_empty_stems_are_pythons():
    rep = node("surface")
    assert set(rep["refused"]) == {"renderPiece", "renderScore", "renderPiecePcm", "renderScorePcm", "renderPieceWav", "renderScoreWav"}
    for call, messages in rep["refused"].items():
        assert messages == [mix.STEMS_NOT_BOOL] * 3, call
    assert rep["names"] == [mix.stem_names(0, 0), mix.stem_names(2, 1), mix.stem_names(8, 4)]
    d.configure(sv.SAMPLE_RATE)
    voices = lambda: [sv.voice(k) for k in range(3)]
    with_tracks = dict(tracks=[mc.echo, None], track_of=[0, 1, -1], faders=[1, 0.5], buses=[mc.comb], track_sends=[[1, 0]])
    empty = d.render_score(voices(), [0, 1, 2], 0.01, 0, stems=True, **with_tracks)
    assert rep["empty"] == {"names": empty.names, "tracks": len(empty.tracks), "buses": len(empty.buses), "mix": len(empty.mix), "sampleRate": empty.mix.sampleRate,
                            "peaks": list(empty.peaks), "peak": float(empty.peak), "gain": not hasattr(empty, "gain")}
    pcm = d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 2, stems=True)
    assert rep["pcm"] == {"names": pcm.names, "tracks": 0, "buses": 0, "bytes": pcm.mix.data.size, "bitDepth": pcm.direct.bitDepth, "gain": float(pcm.gain)}
    assert rep["off"] is True and rep["commonPeak"] == [float(wav.common_peak([0.5, 2, 1])), float(wav.common_peak([])), True]


@pytest.mark.gpu
def test_stems_through_node_are_pythons(tmp_path):
    from test_gpu_stems import loud_case, stacked
    n, rate = 13, sv.SAMPLE_RATE
    d.configure(rate)
    onsets, _, gains = sv.layout(n)
    durations = [((sv.NV if k % 2 == 0 else NV_SAW) + 0.5) / rate for k in range(n)]
    dur = (sv.NT + 0.5) / rate
    of2, of3, f2, f3, levels, sends, pans = tc.track_of(n, 2), tc.track_of(n, 3), tc.faders(2), tc.faders(3), tc.levels(2, 3), sc.levels(n, 1), pans_for(n)
    voices = lambda: [interleaved_voice(k) for k in range(n)]
    mono = lambda: [sv.voice(k) for k in range(n)]
    tracked = dict(tracks=[mc.clip, None, mc.echo], track_of=of3, faders=f3, buses=[mc.echo, mc.comb], track_sends=levels, stems=True)
    calls = {
        ".full": d.render_piece(voices(), onsets, durations, dur, None, gains, **tracked),
        ".master": d.render_piece(voices(), onsets, durations, dur, None, gains, master=mc.comb, **tracked),
        ".sends": d.render_piece(mono(), onsets, durations[0], dur, None, gains, pans=pans, buses=[mc.echo], sends=sends, stems=True),
        ".plain": d.render_piece(voices(), onsets, durations, dur, None, gains, stems=True),
        ".score": d.render_score(mono(), onsets, durations[0], dur, None, gains, tracks=[mc.echo, mc.comb], track_of=of2, faders=f2, stems=True),
    }
    spec = str(tmp_path / "stems.json")
    for tag, got in calls.items():
        stack = stacked(got)
        assert stack.shape[2] == sv.NT and np.abs(stack[-1]).max() > 0
        stack.tofile(spec[:-5] + tag + ".f32")
        np.array([got.peaks[name] for name in got.names], dtype=np.float32).tofile(spec[:-5] + tag + ".peaks.f32")
    make, loud_onsets, loud_gains, loud_of, _ = loud_case()
    pcm = d.render_piece_pcm(make, loud_onsets, durations[0], dur, 16, 2, None, loud_gains, tracks=[None, None], track_of=loud_of, faders=[1, -1], stems=True)
    np.stack([pcm[name].data for name in pcm.names]).tofile(spec[:-5] + ".loud.s16")
    np.array([pcm.peaks[name] for name in pcm.names], dtype=np.float32).tofile(spec[:-5] + ".loud.peaks.f32")
    floats = lambda a: [float(x) for x in a]
    with open(spec, "w") as f:
        json.dump({"n": n, "sampleRate": rate, "onsets": onsets.tolist(), "gains": floats(gains), "voiceDurations": durations, "duration": dur,
                   "trackOf2": of2.tolist(), "trackOf3": of3.tolist(), "faders2": floats(f2), "faders3": floats(f3), "trackSends": [floats(row) for row in levels],
                   "sends": floats(sends[0]), "pans": floats(pans), "loudOnsets": loud_onsets.tolist(), "loudGains": floats(loud_gains), "loudTrackOf": loud_of.tolist(),
                   "loudGain": float(pcm.gain)}, f)
    rep = node("render", spec)
    assert rep["checked"] >= 9 and not rep["failed"], rep["failed"]
