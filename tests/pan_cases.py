"""What the stereo-placement tests share (tests/test_pan_host.py, tests/test_gpu_pan.py, tests/test_js_pan.py): seeded pans per voice
count, the piece as ONE reference circuit with a Pan unit behind every voice, and planted mono rows of mixed lengths."""
import functools

import numpy as np

import dusp_amd as d
import score_voices as sv
from test_piece_host import FMAX, PLANTED

FIXED_PANS = [-1.0, 1.0, 0.0, 1e-40, 0.3, 1.5]  # hard left, hard right, centre, a subnormal f32, inside, outside [-1, 1]


@functools.lru_cache(maxsize=None)
def pans_for(n):
    """pans in [-1, 1) from RandomState(100 + n); voice 0 hard left and, from three voices on, voice 1 hard right and voice 2 centred"""
    pans = (np.random.RandomState(100 + n).random_sample(n) * 2 - 1).astype(np.float32)
    pans[0] = -1.0
    if n > 2:
        pans[1], pans[2] = 1.0, 0.0
    pans.setflags(write=False)
    return pans


def as_one_panned_circuit(voices, onsets, pans, gains=None):
    """The panned piece as the reference would build it: Sum.many of Delay(P_k, onset_k, MAX_DELAY), P_k = Pan(voice_k, pan_k) with the
    voice under Multiply(., g_k) when there are gains; the voice with onset 0 bare (sv.as_one_circuit says why)."""
    if gains is not None:
        voices = [d.Multiply(v, float(g)) for v, g in zip(voices, gains)]
    voices = [d.Pan(v, float(p)) for v, p in zip(voices, pans)]
    return d.Sum.many([v if int(on) == 0 else d.Delay(v, int(on), sv.MAX_DELAY) for v, on in zip(voices, onsets)])


@functools.lru_cache(maxsize=None)
def planted(n, n_total=1301):
    """-> rows (n mono arrays [1, samples_k] of 773, 1, 255, 0, 257 and 3 samples in turn, seeded, scales spanning 1e-3 .. 1e3, with
    test_piece_host's PLANTED values, a subnormal and the largest f32 among them), onsets (both signs; one voice straddles the end, one
    began before the timeline), lengths (0, 1, whole rows and anything between), gains (one negative), pans (FIXED_PANS in turn), init
    [2, n_total] (with -0, inf and NaN)."""
    rng = np.random.RandomState(7000 + n)
    cycle = [773, 1, 255, 0, 257, 3]
    samples = [cycle[k % 6] for k in range(n)]
    rows = [(rng.standard_normal((1, s)) * 10.0 ** (k % 7 - 3)).astype(np.float32) for k, s in enumerate(samples)]
    big = [k for k, s in enumerate(samples) if s >= 255]
    for j, v in enumerate(PLANTED):
        rows[big[j % len(big)]][0, 3 + j] = v
    for k in big:
        rows[k][0, :3] = [-0.0, 5e-39, FMAX]
    onsets = np.array([rng.randint(-max(s, 1), n_total + 2) for s in samples], dtype=np.int64)
    lengths = np.array([rng.randint(0, s + 1) for s in samples], dtype=np.int64)
    lengths[::4] = np.array(samples)[::4]
    onsets[0], lengths[0] = n_total - 20, samples[0]  # straddles the end
    if n > 2:
        onsets[2], lengths[2] = -100, samples[2]      # began before the timeline: a negative onset
    if n > 4:
        onsets[4], lengths[4] = 256 - 7, 257          # across a block boundary
    if n > 1:
        lengths[1] = 1
    gains = (0.05 + 1.9 * rng.random_sample(n)).astype(np.float32)
    if n > 2:
        gains[1] = -gains[1]
    pans = np.array([FIXED_PANS[k % 6] for k in range(n)], dtype=np.float32)
    init = (30 * rng.standard_normal((2, n_total))).astype(np.float32)
    init[0, 5], init[1, 6], init[0, 7], init[1, 1300] = -0.0, np.inf, np.nan, -0.0
    for a in rows + [onsets, lengths, gains, pans, init]:
        a.setflags(write=False)
    return rows, onsets, lengths, gains, pans, init
