"""What the sub-sample-onset tests share (tests/test_frac_host.py, tests/test_gpu_frac.py, tests/test_js_frac.py): onsets and fractions
per voice count, the piece as ONE reference circuit whose Delay units take onset + fraction, and planted rows — mono for the panned form,
of one or two channels for the plain one — with fractions at the edges of [0, 1).

Where the reference anchors the contract, and where the anchor ends:
  * the reference's Delay drops a ceil tap that lands on ring index maxDelay, once a trip round the ring: the circuits here take a ring
    of RING samples, longer than timeline + largest onset + 2, so the ring never wraps (score_voices.MAX_DELAY would);
  * a delay in (0, 1) puts the floor tap into the slot the unit has just read: every voice with a fraction has onset >= 1 here;
  * an inlet constant is rounded to f32: onset + fraction is an f32 here (onsets below 2^12, fractions in 1024ths or 2048ths)."""
import functools

import numpy as np

import dusp_amd as d
import score_voices as sv
from pan_cases import pans_for, planted as pan_planted

RING = 8192
assert RING > sv.NT + sv.NT + 2

EDGE_FRACS = [0.0, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -53, 0.3, 1.0 / 1024, 0.0, 0.999]  # in turn over the planted voices


@functools.lru_cache(maxsize=None)
def layout(n, panned=False):
    """-> onsets int64 [n], fracs float64 [n], gains float32 [n].  sv.layout's onsets and gains; fractions j/1024 with every fifth voice
    at 0, from three voices on one at 0.5 and one at 1/1024 (panned: j/2048, every fourth at 0).  The voice at onset 0 has no fraction (a lone voice is moved
    to onset 5 instead): a voice with a fraction has onset >= 1."""
    onsets, _, gains = sv.layout(n)
    onsets = onsets.copy()
    rs = np.random.RandomState(500 + n + (1000 if panned else 0))
    denom, every = (2048, 4) if panned else (1024, 5)
    fracs = rs.randint(1, denom, n).astype(np.float64) / denom
    fracs[every - 1::every] = 0.0
    if n == 1:
        onsets[0], fracs[0] = 5, 333.0 / denom
    if n > 2:
        fracs[1] = 0.5
    if n > 3:
        fracs[3] = 1.0 / 1024
    fracs[onsets == 0] = 0.0
    assert np.all((fracs == 0) | (onsets >= 1)) and np.all((fracs >= 0) & (fracs < 1))
    assert np.all((onsets + fracs).astype(np.float32).astype(np.float64) == onsets + fracs), "onset + fraction is an f32"
    for a in (onsets, fracs):
        a.setflags(write=False)
    return onsets, fracs, gains


def as_one_frac_circuit(voices, onsets, fracs, gains=None, pans=None):
    """The piece as the reference would build it: Sum.many of Delay(P_k, onset_k + frac_k, RING), P_k the voice under Multiply(., g_k)
    when there are gains and under Pan(., pan_k) when there are pans; the voice at 0 bare (sv.as_one_circuit says why)."""
    if gains is not None:
        voices = [d.Multiply(v, float(g)) for v, g in zip(voices, gains)]
    if pans is not None:
        voices = [d.Pan(v, float(p)) for v, p in zip(voices, pans)]
    at = [float(on) + float(f) for on, f in zip(onsets, fracs)]
    return d.Sum.many([v if a == 0 else d.Delay(v, int(a) if a == int(a) else a, RING) for v, a in zip(voices, at)])


def edge_fracs(n):
    fracs = np.array([EDGE_FRACS[k % len(EDGE_FRACS)] for k in range(n)], dtype=np.float64)
    fracs.setflags(write=False)
    return fracs


@functools.lru_cache(maxsize=None)
def planted(n, n_total=1301):
    """pan_cases.planted — mono rows of 773, 1, 255, 0, 257 and 3 samples in turn with -0, NaN, +-inf, subnormals and the largest f32 among
    them, onsets of both signs, lengths, gains, pans, init [2, n_total] — and fracs [n]: EDGE_FRACS in turn.
    -> rows, onsets, lengths, gains, pans, init, fracs"""
    return pan_planted(n, n_total) + (edge_fracs(n),)


@functools.lru_cache(maxsize=None)
def planted_wide(n, n_total=1301):
    """planted with rows of TWO channels: channel 0 the mono row, channel 1 seeded anew (with a NaN and a -0 of its own)"""
    rows, onsets, lengths, gains, pans, init, fracs = planted(n, n_total)
    rng = np.random.RandomState(9000 + n)
    wide = []
    for k, r in enumerate(rows):
        second = (rng.standard_normal(r.shape) * 10.0 ** ((k + 3) % 7 - 3)).astype(np.float32)
        if r.shape[1] >= 255:
            second[0, 100:104] = [np.nan, -0.0, np.inf, 1e-42]
        w = np.concatenate([r, second], axis=0)
        w.setflags(write=False)
        wide.append(w)
    return wide, onsets, lengths, gains, pans, init, fracs


__all__ = ["RING", "EDGE_FRACS", "layout", "as_one_frac_circuit", "edge_fracs", "planted", "planted_wide", "pans_for"]
