"""What the score tests share (tests/test_score_host.py, tests/test_gpu_score.py): a short voice that ends in exact zeros, a timeline
longer than the voice, and seeded onsets, lengths and gains per voice count."""
import functools

import numpy as np

import dusp_amd as d

SAMPLE_RATE = 48000
NT = 2317  # samples of timeline
NV = 773   # samples a voice is rendered for
MAX_DELAY = 4096


def voice(k):
    return d.Multiply(d.Osc(200.5 + 31 * k), d.Ramp(700, 1, 0).trigger())


@functools.lru_cache(maxsize=None)
def layout(n):
    """-> onsets int64 [n] (voice n // 2 at 0, the others anywhere up to the timeline's last samples: voices straddle its end), lengths
    int64 [n] in 700 .. NV (the Ramp has ended by sample 700: what a length cuts off is zeros), gains float32 [n] (one negative)"""
    rs = np.random.RandomState(n)
    onsets = rs.randint(1, NT - 10, n).astype(np.int64)
    onsets[n // 2] = 0
    lengths = rs.randint(700, NV + 1, n).astype(np.int64)
    gains = (0.05 + 1.9 * rs.random_sample(n)).astype(np.float32)
    if n > 2:
        gains[1] = -gains[1]
    for a in (onsets, lengths, gains):
        a.setflags(write=False)
    return onsets, lengths, gains


def as_one_circuit(voices, onsets, gains=None):
    """The piece as the reference would build it: Sum.many of Delay(voice_k, onset_k, MAX_DELAY), each voice under Multiply(., g_k) when
    there are gains.  The voice with onset 0 stays bare: Delay's `delay || 4410` would make a zero delay 4410 samples."""
    if gains is not None:
        voices = [d.Multiply(v, float(g)) for v, g in zip(voices, gains)]
    return d.Sum.many([v if int(on) == 0 else d.Delay(v, int(on), MAX_DELAY) for v, on in zip(voices, onsets)])
