"""What the stereo-piece tests share (tests/test_stereo_host.py, tests/test_gpu_stereo.py, tests/test_js_stereo.py): voices of the three
kinds — a mono voice behind a Pan, a plain mono voice, a voice of two channels — in three list orders, the piece as ONE reference circuit,
and planted rows of one and two channels with the kinds in turn.

The voices have no Filter and no pow unit, and end in exact zeros before the samples they are rendered for run out (a Ramp), so that
what a row cuts off is zeros.  With fractions the limits of frac_cases hold: a ring longer than the timeline and the largest onset,
onset >= 1 for a voice with a fraction, onset + fraction an f32."""
import functools

import numpy as np

import dusp_amd as d
import score_voices as sv
from frac_cases import RING, edge_fracs, layout as frac_layout
from pan_cases import FIXED_PANS, pans_for, planted as pan_planted

PANNED, MONO, TWO = 0, 1, 2
ORDERS = ["mono_first", "stereo_first", "in_turn"]
NAN = np.float32(np.nan)


def kind_of(k, n, order):
    """mono_first: the first half plain and panned mono in turn (the reference's partial sums are ONE channel wide at first), then two
    channels; stereo_first: the first half two channels, then panned and plain mono in turn; in_turn: panned, plain, two, ..."""
    half = (n + 1) // 2
    if order == "mono_first":
        return (MONO if k % 2 == 0 else PANNED) if k < half else TWO
    if order == "stereo_first":
        return TWO if k < half else (PANNED if (k - half) % 2 == 0 else MONO)
    return (PANNED, MONO, TWO)[k % 3]


def kinds_for(n, order):
    return [kind_of(k, n, order) for k in range(n)]


def voice(k, kind):
    """three structures: the score voice (panned), the score voice under a constant factor (plain mono), the score voice under a pair of
    factors (two channels: Multiply(osc, [a, b]))"""
    if kind == PANNED:
        return sv.voice(k)
    if kind == MONO:
        return d.Multiply(sv.voice(k), 0.625)
    return d.Multiply(sv.voice(k), [0.75 - 0.03125 * (k % 5), -0.5 + 0.0625 * (k % 7)])


def voices_for(n, order):
    return [voice(k, kind) for k, kind in enumerate(kinds_for(n, order))]


@functools.lru_cache(maxsize=None)
def stereo_pans(n, order):
    """pans_for's pans for the panned voices, NaN for the others"""
    pans = np.where(np.array(kinds_for(n, order)) == PANNED, pans_for(n), NAN).astype(np.float32)
    pans.setflags(write=False)
    return pans


def as_one_stereo_circuit(voices, onsets, pans, gains=None, fracs=None):
    """The piece as the reference would build it: Sum.many of Delay(P_k, onset_k + frac_k, RING), P_k the voice under Multiply(., g_k)
    when there are gains and behind Pan(., pan_k) when its pan is a number; the voice at 0 bare (sv.as_one_circuit says why)."""
    if gains is not None:
        voices = [d.Multiply(v, float(g)) for v, g in zip(voices, gains)]
    voices = [v if p is None or np.isnan(p) else d.Pan(v, float(p)) for v, p in zip(voices, pans)]
    at = [float(on) + (float(fracs[k]) if fracs is not None else 0.0) for k, on in enumerate(onsets)]
    return d.Sum.many([v if a == 0 else d.Delay(v, int(a) if a == int(a) else a, RING) for v, a in zip(voices, at)])


def layout(n, with_fracs=False):
    """-> onsets, fracs (None without), gains: sv.layout's, or frac_cases.layout's"""
    if with_fracs:
        return frac_layout(n)
    onsets, _, gains = sv.layout(n)
    return onsets, None, gains


# ---- planted rows -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def planted(n, n_total=1301, kinds="in_turn"):
    """pan_cases.planted's rows — 773, 1, 255, 0, 257 and 3 samples in turn with -0, NaN, +-inf, subnormals and the largest f32 among
    them, onsets of both signs, lengths, gains, init [2, n_total] — as rows of one and two channels, the kinds in turn (kinds: "in_turn",
    or PANNED / MONO / TWO for a list all of one kind): a two-channel row's second channel is seeded anew, with a NaN and a -0 of its own.
    -> rows, onsets, lengths, gains, pans (FIXED_PANS in turn for the panned voices, NaN for the others), init, fracs (frac_cases.EDGE_FRACS
    in turn)"""
    rows, onsets, lengths, gains, pans, init = pan_planted(n, n_total)
    rng = np.random.RandomState(9100 + n)
    which = [(PANNED, MONO, TWO)[k % 3] if kinds == "in_turn" else kinds for k in range(n)]
    out = []
    for k, r in enumerate(rows):
        second = (rng.standard_normal(r.shape) * 10.0 ** ((k + 3) % 7 - 3)).astype(np.float32)
        if r.shape[1] >= 255:
            second[0, 100:104] = [np.nan, -0.0, np.inf, 1e-42]
        w = np.concatenate([r, second], axis=0) if which[k] == TWO else np.array(r)
        w.setflags(write=False)
        out.append(w)
    pans = np.where(np.array(which) == PANNED, pans, NAN).astype(np.float32)
    pans.setflags(write=False)
    return out, onsets, lengths, gains, pans, init, edge_fracs(n)


def edge_rows():
    """a two-channel row of 0 samples and one of 1 sample, beside a mono row: -> rows, onsets, pans"""
    rows = [np.zeros((2, 0), dtype=np.float32), np.array([[1.5], [-2.5]], dtype=np.float32), np.array([[1.0, 2.0, 3.0]], dtype=np.float32)]
    return rows, np.array([2, 4, 3], dtype=np.int64), np.array([NAN, NAN, NAN], dtype=np.float32)


__all__ = ["PANNED", "MONO", "TWO", "ORDERS", "FIXED_PANS", "kinds_for", "voice", "voices_for", "stereo_pans", "as_one_stereo_circuit", "layout", "planted", "edge_rows"]
