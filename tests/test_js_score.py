"""renderScore / renderScorePcm / renderScoreWav of the JavaScript host (dusp_amd/js): voices mixed on the device at per-voice onsets,
through the N-API addon, against the Math.fround chain over renderMany's rows placed at their onsets and against
renderChannelData(Sum.many(Delay ...)) (tests/js/check_score.js)."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "dusp_amd", "js", "addon", "dusp_napi.node")


@pytest.mark.gpu
def test_render_score_through_node():
    assert NODE is not None, "node is needed for the JavaScript host"
    if not os.path.exists(ADDON):
        subprocess.check_call(["make", "-C", os.path.dirname(ADDON), "-s"])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "check_score.js"), "--sampleRate=48000"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, "exit %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-2000:])
    rep = json.loads(lines[-1])
    assert rep.get("fatal") is None, rep
    assert rep["checked"] >= 60 and not rep["failed"], rep["failed"]
