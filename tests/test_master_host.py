"""The master of a score or piece, on the CPU.  The contract is mix.master_chain: the master circuit rendered over the
raw timeline as its one input stream, channel by channel.  The anchor tests hold it to the reference's own way of saying it,
`fx(Sum.many(Delay(voice_k, onset_k, maxDelay)))` rendered as ONE circuit by the CPU oracle — bit for bit on six masters, and they pin
the two places where it is NOT the one circuit (a reconvergent master; the comb family on two channels), so that the documentation
cannot rot unnoticed.  Then the model over planted rows, and the Python surface without a device."""
import functools

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
from dusp_amd import descriptor, mix, render
from dusp_amd.mix import score_chain_rows
from test_piece_host import bits, planted_rows, same


@functools.lru_cache(maxsize=None)
def raw_timeline(n, stereo, oracle):
    """the oracle's renders of the score voices (or the two-channel ones) under sv.layout's onsets and gains, as the chain leaves them"""
    d.configure(sv.SAMPLE_RATE)
    voice = mc.stereo_voice if stereo else sv.voice
    uni = descriptor.unify([descriptor.extract(voice(k)) for k in range(n)])
    rows = [np.asarray(r, dtype=np.float32) for r in oracle.render_instances(uni.words, sv.NV, uni.params, n, range(n))]
    onsets, _, gains = sv.layout(n)
    raw = score_chain_rows(rows, onsets, sv.NT, None, gains, raw=True)
    assert not np.isnan(raw).any() and not np.signbit(raw[raw == 0]).any()  # (NaN-free, and a chain from +0 holds no -0: raw and delivered are the same bits)
    raw.setflags(write=False)
    return raw


def one_circuit(fx, n, stereo, oracle):
    """the reference's expression: fx over Sum.many of the voices' Delays, rendered as ONE circuit"""
    d.configure(sv.SAMPLE_RATE)
    voice = mc.stereo_voice if stereo else sv.voice
    onsets, _, gains = sv.layout(n)
    return np.asarray(oracle.render(mc.words_of(fx(sv.as_one_circuit([voice(k) for k in range(n)], onsets, gains))), sv.NT), dtype=np.float32)


@pytest.mark.parametrize("n", [2, 13])
@pytest.mark.parametrize("name", list(mc.MASTERS))
def test_the_master_over_the_stream_against_the_one_circuit_mono(name, n, oracle):
    fx, equal = mc.MASTERS[name]
    want = one_circuit(fx, n, False, oracle)
    got = mc.oracle_master(oracle, fx, raw_timeline(n, False, oracle))
    assert got.shape == want.shape == (1, sv.NT) and got.dtype == np.float32
    differ = (bits(got) != bits(want)).any(axis=0)
    if equal:
        assert not differ.any(), "first differing sample %d" % int(np.argmax(differ))
    else:  # the reconvergent master: the one circuit's process order places it differently behind a Sum chain than behind a source unit
        assert differ.any() and int(np.argmax(differ)) == 480 and not differ[:480].any()
        # ... by two chunks on the delayed path, exactly: the master with 480 + 512 samples of delay over the stream IS the one circuit
        assert np.array_equal(bits(mc.oracle_master(oracle, mc.reconvergent_two_chunks_late, raw_timeline(n, False, oracle))), bits(want))
    # the stream form through a HostSource unit is the same render as through a MasterInput
    d.configure(sv.SAMPLE_RATE)
    raw = raw_timeline(n, False, oracle)
    ex = descriptor.extract(fx(d.HostSource(raw[0])))
    assert np.array_equal(bits(oracle.render(ex.words, sv.NT, inputs=raw)), bits(got))


@pytest.mark.parametrize("name", list(mc.STEREO_MASTERS))
def test_the_master_over_the_stream_against_the_one_circuit_two_channels(name, oracle):
    fx, equal = mc.MASTERS[name][0], mc.STEREO_MASTERS[name]
    n = 5
    want = one_circuit(fx, n, True, oracle)
    got = mc.oracle_master(oracle, fx, raw_timeline(n, True, oracle))
    assert got.shape == (2, sv.NT)
    if equal:
        assert want.shape == (2, sv.NT) and np.array_equal(bits(got), bits(want))
    else:  # the reference's comb family gives ONE channel for a two-channel input: per-channel application is not the reference there
        assert want.shape == (1, sv.NT)


def test_a_master_a_channel_is_one_program_with_the_constants_as_its_table():
    uni = mc.unified_master([mc.echo_of(300.25), mc.echo_of(411.5)], 2)
    assert uni.n_instances == 2 and uni.n_params == 1 and uni.params.dtype == np.float32 and uni.params.tolist() == [[300.25, 411.5]]
    assert int(uni.words[6]) == 1
    one = mc.unified_master(mc.echo, 3)  # one function: called once per channel, nothing differs
    assert one.n_instances == 3 and one.n_params == 0 and one.params is None
    # the MasterInput is extracted as INPUT stream 0 and carries no samples
    d.configure(sv.SAMPLE_RATE)
    x = d.MasterInput()
    ex = descriptor.extract(mc.clip(x))
    assert ex.sources == [x] and not hasattr(x, "samples")
    assert descriptor.UNITS["MasterInput"] == descriptor.UNITS["HostSource"] == (descriptor.OP_INPUT, [])
    assert np.array_equal(ex.words, descriptor.extract(mc.clip(d.HostSource(np.zeros(3)))).words)
    with pytest.raises(descriptor.DuspError) as e:
        d.renderChannelData(mc.clip(d.MasterInput()), 0.01)
    assert str(e.value) == mix.MASTER_INPUT_ALONE


def test_the_raw_timeline_reaches_the_master_as_it_stands(oracle):
    """planted rows: a NaN, an Inf and a -0 on the raw timeline are what the master is handed; `|| 0` is the master's own copy-out's"""
    rows, onsets, lengths, gains, n_total = planted_rows()
    raw = score_chain_rows(rows, onsets, n_total, lengths, gains, raw=True)
    delivered = score_chain_rows(rows, onsets, n_total, lengths, gains)
    assert np.isnan(raw).any() and np.isinf(raw).any() and raw.shape == (2, n_total)
    heard = []

    def through(c, x):
        heard.append((c, x.copy()))
        return np.where(np.isnan(x), np.float32(0), x)

    out = mix.master_chain(raw, through)
    assert [c for c, _ in heard] == [0, 1] and all(x.dtype == np.float32 and same(x, raw[c]) and np.array_equal(np.signbit(x), np.signbit(raw[c])) for c, x in heard)
    assert out.dtype == np.float32 and out.shape == raw.shape
    # the oracle: x + 1 behind the chain.  Where the chain holds NaN the master's Sum holds NaN and its copy-out delivers 0 — a master over
    # the DELIVERED timeline would have said 1 there; an Inf stays
    got = mc.oracle_master(oracle, lambda x: d.Sum(x, 1), raw)
    nan, inf = np.isnan(raw), np.isinf(raw)
    assert (got[nan] == 0).all() and np.array_equal(got[inf], raw[inf])
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(got[~nan]), bits((raw + np.float32(1))[~nan]))
    over_delivered = mc.oracle_master(oracle, lambda x: d.Sum(x, 1), delivered)
    assert (over_delivered[nan] == 1).all()
    # a master that passes its input on delivers the delivered timeline: `|| 0` once, at the end
    assert same(mc.oracle_master(oracle, lambda x: d.Multiply(x, 1), raw), delivered)
    for bad in (lambda: mix.master_chain(raw.astype(np.float64), through), lambda: mix.master_chain(raw[0], through), lambda: mix.master_chain(raw, lambda c, x: x[:5])):
        with pytest.raises(ValueError, match="dusp-hip"):
            bad()


# ---- the Python surface, without a device ----------------------------------------------------------------------------------------------

def scheduled(x):
    u = mc.clip(x)
    u.schedule(0.01, lambda unit: None)
    return u


REFUSALS = {
    "notCallable": (lambda: 5, 1, mix.MASTER_NOT_CALLABLE),
    "emptyList": (lambda: [], 1, mix.MASTER_NOT_CALLABLE),
    "count": (lambda: [mc.echo], 2, mix.MASTER_COUNT % (1, 2)),
    "noInput": (lambda: (lambda x: sv.voice(0)), 1, mix.MASTER_ONE_INPUT % (0, 0)),
    "twoInputs": (lambda: [mc.echo, lambda x: d.Sum(x, d.MasterInput())], 2, mix.MASTER_ONE_INPUT % (1, 2)),
    "hostSource": (lambda: (lambda x: d.Sum(x, d.HostSource(np.zeros(8)))), 1, mix.MASTER_HOST_SOURCE % 0),
    "events": (lambda: scheduled, 1, mix.MASTER_EVENTS % 0),
    "channels": (lambda: (lambda x: d.Pan(x, 0.25)), 1, mix.MASTER_CHANNELS % (0, 2)),
    "notIsomorphic": (lambda: [mc.echo, mc.echo, mc.clip], 3, mix.MASTER_NOT_ISOMORPHIC % 2),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_what_is_no_master_is_refused_by_string(case):
    master, channels, message = REFUSALS[case]
    d.configure(sv.SAMPLE_RATE)
    with pytest.raises(descriptor.DuspError) as e:
        render.master_program(master(), channels, sv.SAMPLE_RATE)
    assert str(e.value) == message
    assert message.startswith("dusp-hip: ")
    # ... and by every call that takes the keyword, before anything is built (a timeline of no samples needs no device)
    if channels <= 2:
        voices = lambda: [mc.stereo_voice(k) if channels == 2 else sv.voice(k) for k in range(3)]
        for call in (d.render_piece, d.render_score, d.render_piece_pcm, d.render_score_pcm, d.render_piece_wav, d.render_score_wav):
            with pytest.raises(descriptor.DuspError) as e:
                call(voices(), [0, 1, 2], 0.01, 0, master=master())
            assert str(e.value) == message, call.__name__


def test_the_masters_sample_rate_is_the_voices():
    d.configure(44100)
    with pytest.raises(descriptor.DuspError) as e:
        render.master_program(mc.clip, 1, 48000)
    assert str(e.value) == mix.MASTER_RATE % (44100, 48000)
    d.configure(sv.SAMPLE_RATE)


def test_master_travels_with_the_placement_to_the_piece():
    d.configure(sv.SAMPLE_RATE)
    placing = render._placing(None, None, None, None, -3, None, False)
    assert placing["master"] is None and render._placing(None, None, None, None, -3, None, False, mc.echo)["master"] is mc.echo
    voices = lambda: [sv.voice(k) for k in range(3)]
    # without a master the placement carries none
    *_, channels, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, placing)
    assert channels == 1 and place.master is None and "master" not in place.keywords()
    # the master is made once the timeline's channels are known: one instance a channel, whatever gives the channels
    for kw, want in ((dict(), 1), (dict(pans=[0, 0.5, -0.5]), 2), (dict(places=[[0, 0], [1, 1], [2, 0]], speakers=[[-1, 0], [1, 0], [0, 1]]), 3), (dict(stereo=True), 2)):
        placing = render._placing(kw.get("pans"), None, kw.get("places"), kw.get("speakers"), -3, None, kw.get("stereo", False), mc.echo)
        *_, channels, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, placing)
        assert channels == want and place.master.n_instances == want and place.master.sample_rate == sv.SAMPLE_RATE
    # every other refusal of the call comes first
    with pytest.raises(ValueError, match="pans must have shape"):
        d.render_piece(voices(), [0, 1, 2], 0.01, 0.05, pans=[0], master=5)
    # a score with a master goes the piece's way, as one part
    with pytest.raises(descriptor.DuspError, match="the voices of a score are isomorphic circuits"):
        d.render_score([sv.voice(0), mc.stereo_voice(1)], [0, 1], 0.01, 0, master=mc.echo)
    assert len(d.render_score(voices(), [0, 1, 2], 0.01, 0, master=mc.echo)) == 0 and len(d.render_piece(voices(), [0, 1, 2], 0.01, 0, master=[mc.echo])) == 0
    assert d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, master=mc.echo).data.shape == (0, 1)
