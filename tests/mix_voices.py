"""Voices the mix tests share (tests/test_gpu_mix.py): every one isomorphic over k, with per-instance parameters."""
import dusp_amd as d

# kind -> may the mix be held to the ORACLE bit for bit?  (Filter coefficients come through tan(), Pan through pow(): those voices
# are within the path's tolerance of the oracle, and their mix is held to the same program's own render instead.)
KINDS = {"filtered_saw": False, "bright_saw": False, "feedback": False, "pan": False, "fm": True, "osc": True}


def voice(kind, k):
    if kind == "filtered_saw":  # a cutoff per instance, the column on both sides of the scan's lower bound (about 1.5 kHz)
        return d.Filter(d.Osc(110 + 3.25 * k, "saw"), 900 + 40 * k)
    if kind == "bright_saw":    # ... and one whose whole column lies where the compiled kernel runs the Filter as a scan: batch and tiles both scan
        return d.Filter(d.Osc(110 + 3.25 * k, "saw"), 2000 + 40 * k)
    if kind == "feedback":      # BASELINE configs[3]'s voice, a delay per instance (both sides of a chunk)
        s = d.Sum(d.Osc(110 + k / 4), 0)
        f = d.Filter(d.Delay(s, 120 + 17.5 * k, 4096), 2000)
        s.B = d.Multiply(f, 0.5)
        return f
    if kind == "pan":           # two channels
        return d.Pan(d.Osc(200 + 7 * k, "triangle"), -0.9 + 0.025 * k)
    if kind == "fm":            # an FM pair under a Ramp
        return d.Multiply(d.Osc(d.Sum(d.Multiply(d.Osc(3 + k / 4), 40 + k), 220.5 + 10 * k)), d.Ramp(1200, 1, 0.25).trigger())
    if kind == "osc":           # the fused engine's voice
        return d.Osc(100.5 + 13 * k)
    raise KeyError(kind)
