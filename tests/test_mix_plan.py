"""A tile of a mix plans what changes bits as the whole batch does (dusp_amd/csrc/jit_plan.hpp JitBatch::whole_n_inst), on the CPU."""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tiles_of_a_mix_warm_up_and_scan_as_the_whole_batch_does(tmp_path):
    """A long feed-forward Filter circuit renders in warming segments (Filter stage) up to 8 instances a CU and unsplit (scan) above.
    For whole batches on both sides of that, renders on both sides of the shortest that is cut, and the warm-up knob's settings: every
    tile size, the ragged last tile included, plans warm / scan as the one render of the whole batch — and the cases do hold tiles
    that would decide otherwise if planned as batches of their own."""
    import dusp_amd as d
    from dusp_amd import descriptor
    d.configure(48000)
    words = descriptor.extract(d.Filter(d.Osc(220, "saw"), 3000)).words
    path = str(tmp_path / "filter_long.f64")
    np.asarray(words, dtype=np.float64).tofile(path)
    exe = str(tmp_path / "mix_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-o", exe, os.path.join(ROOT, "tests", "native", "mix_plan_check.cpp")])
    p = subprocess.run([exe, path], stdout=subprocess.PIPE)
    out = p.stdout.decode()
    rep = json.loads(out.strip().splitlines()[-1])
    assert p.returncode == 0 and rep["bad"] == 0, out[-4000:]
    assert rep["cases"] >= 500 and rep["warm_wholes"] >= 10 and rep["scan_wholes"] >= 10 and rep["tiles_that_alone_differ"] >= 10, rep
