"""Effect sends on the CPU.  The contract is mix.score_chain_sends (the dry chain untouched, and beside it one send
timeline a bus: every dry term times the voice's level), mix.master_chain per bus and mix.bus_return.  The anchor tests hold it to the
reference's ONE circuit Sum(dryChain, fx(sendChain)) on the CPU oracle and pin, per bus, how that reconvergent graph's process order
makes the send path hear previous chunks — the table of DESIGN.md 6.15, asserted so that it cannot rot.  Then the model over planted
rows, the kernel's text on the host under sanitizers, and the Python surface without a device."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
import send_cases as sc
from dusp_amd import descriptor, mix, render
from dusp_amd.mix import score_chain_rows, score_chain_rows_panned, score_chain_sends
from test_piece_host import ROOT, SANITIZE, bits, planted_rows, same

# DESIGN.md 6.15's anchor table.  name -> n -> (is the contract the one circuit bit for bit?, the chunks by which voice k's SEND path is
# late in the one circuit).  The dry path is never late.
ANCHOR = {
    "echo": {2: (True, [1, 0]), 13: (False, [6, 5, 5, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1])},
    "comb": {2: (False, [2, 1]), 13: (False, [6, 5, 5, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1])},
    "clip": {2: (False, [3, 2]), 13: (False, [7, 6, 6, 6, 6, 5, 5, 4, 4, 3, 3, 2, 2])},
}
CHUNK = 256


@functools.lru_cache(maxsize=None)
def voice_rows(n, oracle):
    d.configure(sv.SAMPLE_RATE)
    uni = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(n)])
    rows = tuple(np.asarray(r, dtype=np.float32) for r in oracle.render_instances(uni.words, sv.NV, uni.params, n, range(n)))
    for r in rows:
        r.setflags(write=False)
    return rows


@pytest.mark.parametrize("n", [2, 13])
@pytest.mark.parametrize("name", list(ANCHOR))
def test_the_contract_against_the_one_circuit(name, n, oracle):
    fx = sc.BUSES[name]
    equal, send_lags = ANCHOR[name][n]
    d.configure(sv.SAMPLE_RATE)
    onsets, _, gains = sv.layout(n)
    levels = sc.levels(n)
    one = sc.OneCircuit(fx, [sv.voice(k) for k in range(n)], onsets, gains, levels[0])
    ex = descriptor.extract(one.out)
    want = np.asarray(oracle.render(ex.words, sv.NT), dtype=np.float32)
    rows = list(voice_rows(n, oracle))
    got, dry = sc.expected(oracle, rows, onsets, sv.NT, [fx], levels, gains=gains)
    assert got.shape == want.shape == (1, sv.NT) and got.dtype == np.float32
    assert (bits(got) != bits(dry)).sum() > 500  # (the bus is heard)
    assert np.array_equal(bits(got), bits(want)) == equal
    # what the one circuit's process order does: the table's lags are the circuit's own ...
    dry_lags, lags = sc.chunk_lags(one, {u: i for i, u in enumerate(ex.circuit.units)})
    assert dry_lags == [0] * n and lags == send_lags
    # ... and the one circuit IS the contract with voice k's send so many chunks late, bit for bit: the dry chain as it stands, the
    # send chain over onsets moved by the lags, the bus over that, the return
    d.configure(sv.SAMPLE_RATE)
    raw, _ = score_chain_sends(rows, onsets, sv.NT, levels, None, gains)
    _, late = score_chain_sends(rows, onsets + CHUNK * np.array(lags), sv.NT, levels, None, gains)
    assert np.array_equal(bits(mix.bus_return(raw, [mc.oracle_master(oracle, fx, late[0])])), bits(want))


def test_the_send_chain_is_every_dry_term_times_the_level():
    rows, onsets, lengths, gains, n_total = planted_rows()
    n = len(rows)
    rs = np.random.RandomState(3)
    sends = (rs.random_sample((3, n)) * 2 - 0.5).astype(np.float32)
    sends[1, ::3] = 0
    for g in (None, gains):
        dry, send = score_chain_sends(rows, onsets, n_total, sends, lengths, g)
        assert dry.dtype == send.dtype == np.float32 and dry.shape == (2, n_total) and send.shape == (3, 2, n_total)
        assert np.array_equal(bits(dry), bits(score_chain_rows(rows, onsets, n_total, lengths, g, raw=True)))
        # a plain loop: one f32 product and one f32 add a voice, in index order, every voice in every bus's chain
        want = np.zeros((3, 2, n_total), dtype=np.float32)
        with np.errstate(all="ignore"):
            for k, row in enumerate(rows):
                t0, t1 = max(int(onsets[k]), 0), min(int(onsets[k]) + int(lengths[k]), n_total)
                if t1 <= t0:
                    continue
                x = row[:, t0 - int(onsets[k]):t1 - int(onsets[k])]
                term = x * g[k] if g is not None else x
                for b in range(3):
                    want[b, :, t0:t1] = want[b, :, t0:t1] + term * sends[b, k]
        assert same(send, want) and np.array_equal(np.signbit(send), np.signbit(want))
    # two roundings, not one: the send term is f32(f32(x * g) * s), which is not f32(x * (g * s)) everywhere
    with np.errstate(all="ignore"):
        _, folded = score_chain_sends(rows, onsets, n_total, np.ones((1, n), dtype=np.float32), lengths, gains * sends[0])
    _, send = score_chain_sends(rows, onsets, n_total, sends[:1], lengths, gains)
    assert (bits(folded) != bits(send)).any()
    # a level of 1 everywhere: the bus hears the dry chain
    dry, send = score_chain_sends(rows, onsets, n_total, np.ones((1, n), dtype=np.float32), lengths, gains)
    assert same(send[0], dry)
    # one bus: a 1-D array will do
    assert same(score_chain_sends(rows, onsets, n_total, sends[0], lengths, gains)[1], send_of(rows, onsets, n_total, sends[:1], lengths, gains))


def send_of(*args):
    return score_chain_sends(*args)[1]


def test_the_panned_send_chain_is_post_pan():
    rows, onsets, lengths, gains, n_total = planted_rows(n_ch=1)
    n = len(rows)
    pans = np.linspace(-1, 1, n).astype(np.float32)
    sends = sc.levels(n, 2)
    dry, send = score_chain_sends(rows, onsets, n_total, sends, lengths, gains, pans)
    assert dry.shape == (2, n_total) and send.shape == (2, 2, n_total)
    assert np.array_equal(bits(dry), bits(score_chain_rows_panned(rows, onsets, pans, n_total, lengths, gains, raw=True)))
    # voice by voice: its two f32 Pan values, alone on a timeline, times its level
    want = np.zeros_like(send)
    with np.errstate(all="ignore"):
        for k in range(n):
            alone = score_chain_rows_panned([rows[k]], onsets[k:k + 1], pans[k:k + 1], n_total, lengths[k:k + 1], gains[k:k + 1], raw=True)
            t0, t1 = max(int(onsets[k]), 0), min(int(onsets[k]) + int(lengths[k]), n_total)
            for b in range(2):
                want[b, :, t0:t1] = want[b, :, t0:t1] + alone[:, t0:t1] * sends[b, k]
    assert same(send, want)


def test_a_level_of_zero_is_a_multiplication_by_zero():
    """every voice is in every bus's chain: NaN * 0 poisons the bus where the voice sounds, and -x * 0 is -0 — no skipped add"""
    x = np.array([[1.0, np.nan, -2.0, np.inf, 3.0]], dtype=np.float32)
    y = np.array([[-5.0, -6.0]], dtype=np.float32)
    dry, send = score_chain_sends([x, y], [2, 10], 16, [[0.0, 0.0]])
    assert np.isnan(send[0, 0, 3]) and np.isnan(send[0, 0, 5])  # NaN * 0 and Inf * 0
    assert send[0, 0, 2] == 0 and send[0, 0, 4] == 0 and not np.signbit(send[0, 0, 2])  # +0 + (1 * 0), +0 + (-2 * 0 = -0) = +0
    _, minus = score_chain_sends([y], [10], 16, [[0.0]])
    assert (minus[0, 0, 10:12] == 0).all() and not np.signbit(minus[0, 0, 10:12]).any()  # (a chain from +0: +0 + -0 = +0)
    _, neg = score_chain_sends([y], [10], 16, [[-0.0]])
    assert not np.signbit(neg[0, 0, 10:12]).any() and np.isnan(dry[0, 3])
    # the poisoned bus: its render delivers 0 where its circuit holds NaN, and the dry sample survives (the divergence below)
    assert not np.isnan(send[0, 0, [0, 1, 2, 4, 6, 7]]).any()


def test_where_a_bus_puts_out_nan_the_dry_sample_survives(oracle):
    """The ONE divergence that comes from rendering a bus as a program of its own: a NaN on the send timeline is a NaN in the bus, whose
    copy-out makes it 0; the return adds 0 and the dry sample is delivered.  The reference's final Sum would hold NaN there and
    deliver 0.  A planted NaN pins it, as test_the_raw_timeline_reaches_the_master_as_it_stands does for the master."""
    d.configure(sv.SAMPLE_RATE)
    n_total = 64
    clean = np.linspace(0.1, 0.9, 32, dtype=np.float32)[None]
    poison = np.zeros((1, 8), dtype=np.float32)
    poison[0, 2] = np.nan
    rows, onsets = [clean, poison], [4, 10]
    # the poisoned voice is silent in the dry mix by its gain of 0?  No: NaN * 0 is NaN there too.  It sends at level 1 and the clean voice at 0.5
    dry, send = score_chain_sends(rows, onsets, n_total, [[0.5, 1.0]])
    t = 12
    assert np.isnan(send[0, 0, t]) and np.isnan(dry[0, t])
    # ... so take the dry chain of the clean voice alone, and the poisoned send timeline: the bus passes its input on (x * 1)
    dry = score_chain_rows([clean], [4], n_total, raw=True)
    wet = mc.oracle_master(oracle, lambda x: d.Multiply(x, 1), send[0])
    assert wet[0, t] == 0 and not np.isnan(wet).any()  # `|| 0` at the bus's own copy-out
    out = mix.bus_return(dry, [wet])
    assert out[0, t] == dry[0, t] != 0  # the dry sample survives
    with np.errstate(all="ignore"):
        reference = mix.bus_return(dry, [send[0]])  # what the one circuit's final Sum would deliver: NaN || 0
    assert reference[0, t] == 0
    others = np.arange(n_total) != t
    assert np.array_equal(bits(out[0, others]), bits(reference[0, others]))


def test_bus_return_is_sum_many_left_deep():
    rs = np.random.RandomState(5)
    dry = (rs.standard_normal((2, 300)) * 1e3).astype(np.float32)
    wets = [(rs.standard_normal((2, 300)) * 10.0 ** e).astype(np.float32) for e in (-3, 4, 0)]
    dry[0, 5], wets[0][0, 5] = 1.0, -1.0
    dry[1, 7] = -0.0  # (-0 + -0 + -0 + -0 = -0: raw keeps it, `|| 0` does not)
    for w in wets:
        w[1, 7] = -0.0
    dry[0, 9] = np.nan
    want = ((dry + wets[0]) + wets[1]) + wets[2]
    raw = mix.bus_return(dry, wets, raw=True)
    assert raw.dtype == np.float32 and same(raw, want) and np.signbit(raw[1, 7]) and np.isnan(raw[0, 9])
    out = mix.bus_return(dry, wets)
    assert out[0, 9] == 0 and not np.signbit(out[1, 7]) and np.array_equal(bits(out[~np.isnan(want) & (want != 0)]), bits(want[~np.isnan(want) & (want != 0)]))
    assert (bits(raw) != bits(dry + (wets[0] + (wets[1] + wets[2])))).any()  # (the order matters)
    assert same(mix.bus_return(dry, [], raw=True), dry)
    for bad in (lambda: mix.bus_return(dry.astype(np.float64), wets), lambda: mix.bus_return(dry[0], wets), lambda: mix.bus_return(dry, [wets[0][:, :5]])):
        with pytest.raises(ValueError, match="dusp-hip"):
            bad()


def test_check_sends():
    s = mix.check_sends([[0, 0.5, 1], [1, 2, 3]], 3, 2)
    assert s.dtype == np.float32 and s.shape == (2, 3) and s.flags.c_contiguous
    assert mix.check_sends([0.25, 0.5, 1], 3, 1).shape == (1, 3)
    assert mix.check_sends(np.asfortranarray(np.ones((4, 3))), 3, 4).flags.c_contiguous
    for sends, n, buses, message in (
            ([[1, 2, 3]], 3, 0, mix.BUS_COUNT % 0), (np.ones((5, 3)), 3, 5, mix.BUS_COUNT % 5),
            ([1, 2, 3], 3, 2, mix.SENDS_SHAPE % (2, 3)), ([[1, 2]], 3, 1, mix.SENDS_SHAPE % (1, 3)), (np.ones((2, 3, 1)), 3, 2, mix.SENDS_SHAPE % (2, 3)),
            ([[1, 2, 3], [1, np.nan, 3]], 3, 2, mix.SENDS_NOT_FINITE % (1, 1)), ([[1, 2, np.inf]], 3, 1, mix.SENDS_NOT_FINITE % (2, 0)),
            ([[1, 2, 1e39]], 3, 1, mix.SENDS_NOT_FINITE % (2, 0))):
        with pytest.raises(ValueError) as e:
            mix.check_sends(sends, n, buses)
        assert str(e.value) == message and message.startswith("dusp-hip: ")


# ---- the kernel's text, under sanitizers ------------------------------------------------------------------------------------------------

def test_score_send_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/score_send_engine.hip itself, compiled for the host with its lanes run one after the other, every row a heap
    allocation of exactly its size, under AddressSanitizer and UBSan, beside the rows and pan kernels whose dry output it must give
    bit for bit; and the return kernel (tests/native/score_send_kernel_check.cpp lists what it covers)."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "score_send_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub"), "-x", "c++",
                           os.path.join(native, "score_send_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["dry_bad"] == 0 and rep["cases"] > 5000 and rep["doubled"] >= 100 and rep["windows"] >= 100 and rep["zero_first"] >= 1000, rep
    assert rep["returns"] == 200, rep


# ---- the Python surface, without a device ------------------------------------------------------------------------------------------------

CALLS = (d.render_piece, d.render_score, d.render_piece_pcm, d.render_score_pcm, d.render_piece_wav, d.render_score_wav)


def voices(n=3):
    return [sv.voice(k) for k in range(n)]


@pytest.mark.parametrize("call", CALLS, ids=lambda c: c.__name__)
def test_what_does_not_go_with_sends_is_refused_by_string(call):
    d.configure(sv.SAMPLE_RATE)
    s = [0.5, 0, 1]
    for kw, message in ((dict(sends=s), mix.SENDS_WITHOUT_BUSES), (dict(buses=[mc.echo]), mix.BUSES_WITHOUT_SENDS),
                        (dict(buses=[], sends=s), mix.BUS_COUNT % 0), (dict(buses=[mc.echo] * 5, sends=np.ones((5, 3))), mix.BUS_COUNT % 5),
                        (dict(buses=mc.echo, sends=s), mix.BUS_COUNT % 0),
                        (dict(buses=[mc.echo], sends=s, fracs=[0, 0, 0]), mix.SENDS_PLACEMENT),
                        (dict(buses=[mc.echo], sends=s, places=[[0, 0], [1, 1], [2, 0]], speakers=[[-1, 0], [1, 0]]), mix.SENDS_PLACEMENT),
                        (dict(buses=[mc.echo], sends=s, stereo=True), mix.SENDS_PLACEMENT),
                        (dict(buses=[mc.echo], sends=[0.5, 1]), mix.SENDS_SHAPE % (1, 3)),
                        (dict(buses=[mc.echo, mc.clip], sends=s), mix.SENDS_SHAPE % (2, 3)),
                        (dict(buses=[mc.echo], sends=[0.5, np.inf, 1]), mix.SENDS_NOT_FINITE % (1, 0))):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0, **kw)
        assert str(e.value) == message, kw


def scheduled(x):
    u = mc.clip(x)
    u.schedule(0.01, lambda unit: None)
    return u


BUS_REFUSALS = {
    "notCallable": (lambda: 5, 1, mix.BUS_NOT_CALLABLE % 1),
    "emptyList": (lambda: [], 1, mix.BUS_NOT_CALLABLE % 1),
    "count": (lambda: [mc.echo], 2, mix.BUS_CIRCUITS % (1, 1, 2)),
    "noInput": (lambda: (lambda x: sv.voice(0)), 1, mix.BUS_ONE_INPUT % (1, 0, 0)),
    "hostSource": (lambda: (lambda x: d.Sum(x, d.HostSource(np.zeros(8)))), 1, mix.BUS_HOST_SOURCE % (1, 0)),
    "events": (lambda: scheduled, 1, mix.BUS_EVENTS % (1, 0)),
    "channels": (lambda: (lambda x: d.Pan(x, 0.25)), 1, mix.BUS_CHANNELS % (1, 0, 2)),
    "notIsomorphic": (lambda: [mc.echo, mc.clip], 2, mix.BUS_NOT_ISOMORPHIC % (1, 1)),
}


@pytest.mark.parametrize("case", list(BUS_REFUSALS))
def test_what_is_no_bus_is_refused_by_string(case):
    """a bus is held to a master's rules, in a master's words with "bus b" for the noun; bus 1 of two is the one at fault"""
    bus, channels, message = BUS_REFUSALS[case]
    d.configure(sv.SAMPLE_RATE)
    with pytest.raises(descriptor.DuspError) as e:
        render.master_program(bus(), channels, sv.SAMPLE_RATE, bus=1)
    assert str(e.value) == message and message.startswith("dusp-hip: ") and "bus 1" in message
    kw = dict(pans=[0, 0.5, -0.5]) if channels == 2 else {}
    for call in CALLS:
        with pytest.raises(descriptor.DuspError) as e:
            call(voices(), [0, 1, 2], 0.01, 0, buses=[mc.echo, bus()], sends=np.ones((2, 3)), **kw)
        assert str(e.value) == message, call.__name__
    d.configure(44100)
    with pytest.raises(descriptor.DuspError) as e:
        render.master_program(mc.clip, 1, 48000, bus=2)
    assert str(e.value) == mix.BUS_RATE % (2, 44100, 48000)
    d.configure(sv.SAMPLE_RATE)


def test_buses_and_sends_travel_with_the_placement_to_the_piece():
    d.configure(sv.SAMPLE_RATE)
    placing = render._placing(None, None, None, None, -3, None, False)
    assert placing["buses"] is None and placing["sends"] is None
    *_, channels, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, placing)
    assert place.buses is None and place.sends is None and "buses" not in place.keywords() and "sends" not in place.keywords()
    # the buses are made once the timeline's channels are known: one instance a channel each, the levels checked
    for kw, want in ((dict(), 1), (dict(pans=[0, 0.5, -0.5]), 2)):
        placing = render._placing(kw.get("pans"), None, None, None, -3, None, False, None, [mc.echo, [mc.echo_of(300.25)] * want], [[0, 1, 0.5], [1, 1, 1]])
        *_, channels, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, placing)
        assert channels == want and [b.n_instances for b in place.buses] == [want, want] and place.master is None
        assert place.sends.dtype == np.float32 and place.sends.tolist() == [[0, 1, 0.5], [1, 1, 1]]
    # with a master beside them
    placing = render._placing(None, None, None, None, -3, None, False, mc.clip, [mc.echo], [0, 1, 0.5])
    *_, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, placing)
    assert place.master.n_instances == 1 and len(place.buses) == 1 and place.sends.shape == (1, 3)
    # every other refusal of the call comes first; the master's before the buses'
    with pytest.raises(ValueError, match="pans must have shape"):
        d.render_piece(voices(), [0, 1, 2], 0.01, 0.05, pans=[0], buses=[5], sends=[1, 1, 1])
    with pytest.raises(descriptor.DuspError) as e:
        d.render_piece(voices(), [0, 1, 2], 0.01, 0.05, master=5, buses=[5], sends=[1, 1, 1])
    assert str(e.value) == mix.MASTER_NOT_CALLABLE
    # a score with buses goes the piece's way, as one part
    with pytest.raises(descriptor.DuspError, match="the voices of a score are isomorphic circuits"):
        d.render_score([sv.voice(0), mc.stereo_voice(1)], [0, 1], 0.01, 0, buses=[mc.echo], sends=[1, 1])
    assert len(d.render_score(voices(), [0, 1, 2], 0.01, 0, buses=[mc.echo], sends=[1, 0, 1])) == 0
    assert len(d.render_piece(voices(), [0, 1, 2], 0.01, 0, buses=[[mc.echo]], sends=[[1, 0, 1]])) == 0
    assert d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, buses=[mc.echo], sends=[1, 0, 1]).data.shape == (0, 1)
