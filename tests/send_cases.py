"""What the send tests share (tests/test_sends_host.py, tests/test_gpu_sends.py, tests/test_js_sends.py): the buses of DESIGN.md 6.15's
anchor table (the echo, comb and clip of master_cases), level columns, the reference's ONE circuit Sum(dryChain, fx(sendChain)) over
shared Delay units, and the expected value of a call with buses: mix.score_chain_sends over the voices' rows, every bus rendered over
its send timeline by the CPU oracle (master_cases.oracle_master), mix.bus_return."""
import numpy as np

import dusp_amd as d
import master_cases as mc
import score_voices as sv
from dusp_amd import mix

BUSES = {"echo": mc.echo, "comb": mc.comb, "clip": mc.clip}


def levels(n, n_buses=1, zero_column=None, seed=0):
    """-> float32 [n_buses, n]: distinct columns in [-0.5, 1.5), a few voices at exactly 0 in each, one bus all zero on request"""
    rs = np.random.RandomState(100 * n + n_buses + seed)
    s = (rs.random_sample((n_buses, n)) * 2 - 0.5).astype(np.float32)
    s[:, ::4] = 0
    if n > 1:
        s[0, 1] = 0.6
    if zero_column is not None:
        s[zero_column] = 0
    s.setflags(write=False)
    return s


class OneCircuit:
    """The piece with one bus as the reference would build it, ONE circuit: both chains over the SAME Delay units — score_voices'
    as_one_circuit's, Delay(Multiply(v_k, g_k), onset_k), the voice with onset 0 bare — the send chain's links Multiply(., s_k):
        out = Sum(Sum.many(units), fx(Sum.many(Multiply(unit_k, s_k))))
    with the handles chunk_lags needs"""

    def __init__(self, fx, voices, onsets, gains, sends):
        if gains is not None:
            voices = [d.Multiply(v, float(g)) for v, g in zip(voices, gains)]
        self.units = [v if int(on) == 0 else d.Delay(v, int(on), sv.MAX_DELAY) for v, on in zip(voices, onsets)]
        self.dry_last = d.Sum.many(self.units)
        links = [d.Multiply(u, 1) for u in self.units]
        for link, s in zip(links, sends):
            link.B = float(s)  # (set afterwards: the constructor's `b || 1` would make a level of 0 a level of 1)
        self.send_last = d.Sum.many(links)
        self.wet = fx(self.send_last)
        self.out = d.Sum(self.dry_last, self.wet)


def chunk_lags(one, order):
    """What the reference's process order makes of a OneCircuit: a unit that is ticked BEFORE the unit it reads hears that unit's
    previous chunk.  order: unit -> its place in the circuit's process order.  -> (dry lags [voices], send lags [voices], wet lag), in
    chunks: how many such late edges lie on voice k's way to the dry chain's end and into the final Sum; on its way through its send
    link and the send chain into the bus's first unit; and between the bus's output and the final Sum."""
    late = lambda a, b: int(order[a] > order[b])

    def way(a, b, seen):  # the late edges on the one forward path from a to b (None: there is none)
        if a is b:
            return 0
        seen.add(a)
        for nxt in a.outputUnits:
            if nxt not in seen:
                rest = way(nxt, b, seen)
                if rest is not None:
                    return late(a, nxt) + rest
        return None

    dry = [way(u, one.dry_last, set()) + late(one.dry_last, one.out) for u in one.units]
    send = [way(u, one.wet, {one.dry_last}) + late(one.wet, one.out) for u in one.units]
    return dry, send


def expected(oracle, rows, onsets, n_total, buses, sends, lengths=None, gains=None, pans=None, master=None):
    """-> (the delivered mix float32 [C, n_total], the dry mix as delivered without buses): the contract, with the CPU oracle as every
    bus's (and the master's) render.  buses: a list of functions fx(x), or of lists of one a channel"""
    dry, send = mix.score_chain_sends(rows, onsets, n_total, sends, lengths, gains, pans)
    wets = [mc.oracle_master(oracle, fx, send[b]) for b, fx in enumerate(buses)]
    out = mix.bus_return(dry, wets, raw=master is not None)
    if master is not None:
        out = mc.oracle_master(oracle, master, out)
    return out, mix.bus_return(dry, [])
