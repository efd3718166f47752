"""What the track tests share (tests/test_tracks_host.py, tests/test_gpu_tracks.py, tests/test_js_tracks.py): the track circuits of
DESIGN.md 6.16's anchor table (master_cases' clip, echo, comb, allpass and lowpass), where the voices go, faders and levels, the
reference's ONE circuit — a tree, every voice in exactly one track — and the expected value of a call with tracks: the contract's
chains over the voices' rows, destination by destination, every track circuit rendered over its sub-mix by the CPU oracle
(master_cases.oracle_master), mix.track_mix, the buses, the master."""
import numpy as np

import dusp_amd as d
import master_cases as mc
import score_voices as sv
from dusp_amd import descriptor, mix, render

TRACKS = {"clip": mc.clip, "echo": mc.echo, "comb": mc.comb, "allpass": mc.allpass, "lowpass": mc.lowpass}


def track_of(n, n_tracks, direct=True, seed=0):
    """-> int32 [n]: every track has a voice where n allows it, tracks interleave along the voice list, and — direct — about a third of
    the voices go straight to the mix (-1), the voice at onset 0 (n // 2) among them"""
    rs = np.random.RandomState(1000 * n + 10 * n_tracks + seed)
    of = rs.randint(-1 if direct else 0, n_tracks, n).astype(np.int32)
    of[:n_tracks] = np.arange(n_tracks)[:n]
    if direct and n > n_tracks:
        of[n // 2 if n // 2 >= n_tracks else n - 1] = -1
    of.setflags(write=False)
    return of


def faders(n_tracks):
    f = np.array([0.75, -1.25, 0.5, 1.0, 0.3, 1.5, -0.6, 0.9], dtype=np.float32)[:n_tracks]
    f.setflags(write=False)
    return f


def levels(n_buses, n_tracks, zero_column=None):
    """-> float32 [n_buses, n_tracks]: distinct levels in [-0.5, 1.5), one bus all zero on request"""
    rs = np.random.RandomState(100 * n_buses + n_tracks)
    s = (rs.random_sample((n_buses, n_tracks)) * 2 - 0.5).astype(np.float32)
    if zero_column is not None:
        s[zero_column] = 0
    s.setflags(write=False)
    return s


def one_circuit(fxs, voices, onsets, gains, of, fader_values=None):
    """The piece as the reference would build it, ONE circuit, a tree:
        Sum.many([Sum.many(direct voices), Multiply(fx_0(Sum.many(voices of track 0)), f_0), ...])
    each voice Delay(Multiply(v_k, g_k), onset_k), the voice with onset 0 bare (score_voices.as_one_circuit); without direct voices the
    outer Sum.many is over the tracks alone.  A group of one voice is that voice (Sum.many of one)."""
    if gains is not None:
        voices = [d.Multiply(v, float(g)) for v, g in zip(voices, gains)]
    units = [v if int(on) == 0 else d.Delay(v, int(on), sv.MAX_DELAY) for v, on in zip(voices, onsets)]
    group = lambda g: d.Sum.many([u for u, t in zip(units, of) if t == g])
    terms = [group(-1)] if any(t == -1 for t in of) else []
    for g, fx in enumerate(fxs):
        y = fx(group(g))
        if fader_values is not None:
            m = d.Multiply(y, 1)
            m.B = float(fader_values[g])  # (set afterwards: the constructor's `b || 1` would make a fader of 0 a fader of 1)
            y = m
        terms.append(y)
    return d.Sum.many(terms)


def oracle_voice_rows(oracle, voices, voice_samples):
    """the oracle's render of every voice of a list, PART BY PART as a piece renders them -> a list of float32 [channels_k, samples_k]"""
    d.configure(sv.SAMPLE_RATE)
    grouped = render.piece_parts([descriptor.extract(v) for v in voices], voice_samples)
    per_part = [np.stack(oracle.render_instances(uni.words, n_voice, uni.params, uni.n_instances, range(uni.n_instances))).astype(np.float32) for uni, n_voice in grouped.parts]
    return [per_part[p][i] for p, i in zip(grouped.part_of, grouped.instance_of)]


def sub_chain(rows, onsets, n_total, which, channels, lengths=None, gains=None, pans=None, fracs=None, taps=None, stereo=False):
    """the contract's chain — the SAME function the call's placement uses — over the voices `which` alone, in index order, raw;
    zeros [channels, n_total] where there are none"""
    which = [int(k) for k in which]
    if not which:
        return np.zeros((channels, n_total), dtype=np.float32)
    pick = lambda a: None if a is None else np.asarray(a)[which]
    r, on, ln, g, f = [rows[k] for k in which], pick(onsets), pick(lengths), pick(gains), pick(fracs)
    if taps is not None:
        out = mix.score_chain_rows_placed(r, on, pick(taps[0]), pick(taps[1]), n_total, ln, g, None, True)
    elif stereo:
        out = mix.score_chain_rows_stereo(r, on, pick(pans), n_total, ln, g, None, True, None, f)
    elif pans is not None:
        out = mix.score_chain_rows_panned(r, on, pick(pans), n_total, ln, g, None, True, None, f)
    else:
        out = mix.score_chain_rows(r, on, n_total, ln, g, None, True, f)
    assert out.shape == (channels, n_total)
    return out


def expected(oracle, rows, onsets, n_total, fxs, of, channels=1, fader_values=None, lengths=None, gains=None, buses=None, track_sends=None, master=None, **placement):
    """-> the delivered mix float32 [channels, n_total]: the contract, with the CPU oracle as every track's (bus's, master's) render.
    fxs: a list of functions fx(x), of lists of one a channel, or None for a track without a circuit"""
    chain = lambda g: sub_chain(rows, onsets, n_total, np.flatnonzero(np.asarray(of) == g), channels, lengths, gains, **placement)
    direct = chain(-1)
    ys = [chain(g) if fx is None else mc.oracle_master(oracle, fx, chain(g)) for g, fx in enumerate(fxs)]
    out, feeds = mix.track_mix(direct, ys, fader_values, track_sends)
    wets = [mc.oracle_master(oracle, fx, feeds[b]) for b, fx in enumerate(buses or [])]
    out = mix.bus_return(out, wets, raw=master is not None)
    return mc.oracle_master(oracle, master, out) if master is not None else out
