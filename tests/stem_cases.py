"""What the stem tests share (tests/test_stems_host.py, tests/test_gpu_stems.py, tests/test_js_stems.py): the expected value of a call
with stems=True, built from track_cases.expected's pieces — the contract's chain per destination (track_cases.sub_chain), every track
circuit, bus and master rendered by the CPU oracle (master_cases.oracle_master), mix.track_terms, mix.track_mix, mix.bus_return,
mix.stems — or, for per-note sends without tracks, from mix.score_chain_sends; and the two tracks at faders +1 and -1 over nearly the
same voices whose stems are louder than the mix."""
import numpy as np

import master_cases as mc
import track_cases as tc
from dusp_amd import mix


def expected(oracle, rows, onsets, n_total, fxs=None, of=None, channels=1, fader_values=None, lengths=None, gains=None, buses=None, track_sends=None, sends=None, master=None,
             **placement):
    """-> the signals float32 [S + 1, channels, n_total] of the call, mix.stem_names' order.  fxs (None: no tracks): as
    track_cases.expected takes them, with `of` and track_sends; sends (without tracks): the voices' levels [buses, voices], plain rows
    or pans= alone; neither: one timeline, direct and mix."""
    if fxs is not None:
        chain = lambda g: tc.sub_chain(rows, onsets, n_total, np.flatnonzero(np.asarray(of) == g), channels, lengths, gains, **placement)
        direct = chain(-1)
        ys = [chain(g) if fx is None else mc.oracle_master(oracle, fx, chain(g)) for g, fx in enumerate(fxs)]
        terms = mix.track_terms(ys, fader_values)
        out, feeds = mix.track_mix(direct, ys, fader_values, track_sends)
    elif buses:
        assert set(placement) <= {"pans"}
        direct, feeds = mix.score_chain_sends(rows, onsets, n_total, sends, lengths, gains, placement.get("pans"))
        terms, out = [], direct
    else:
        direct = tc.sub_chain(rows, onsets, n_total, range(len(rows)), channels, lengths, gains, **placement)
        terms, out, feeds = [], direct, None
    wets = [mc.oracle_master(oracle, fx, feeds[b]) for b, fx in enumerate(buses or [])]
    out = mix.bus_return(out, wets, raw=master is not None)
    if master is not None:
        out = mc.oracle_master(oracle, master, out)
    return mix.stems(direct, terms, wets, out)


def opposed(n):
    """-> (track_of int32 [n], faders): two fader groups over the SAME kind of voices at faders +1 and -1 — voice 2j on track 0 and voice
    2j + 1 on track 1 — and no direct voices: the tracks cancel in part, and each stem is louder than the mix"""
    of = (np.arange(n) % 2).astype(np.int32)
    of.setflags(write=False)
    return of, np.array([1.0, -1.0], dtype=np.float32)
