"""What the master tests share (tests/test_master_host.py, tests/test_gpu_master.py, tests/test_js_master.py): the seven masters of
DESIGN.md 6.14's anchor table, each a function fx(x) that works alike over a MasterInput (the master of a call), over a HostSource (the
stream form) and over Sum.many of the voices' Delays (the reference's one circuit); and the expected value of a call with a master,
mix.master_chain with the CPU oracle as the master's render."""
import numpy as np

import dusp_amd as d
import mix_voices
import score_voices as sv
from dusp_amd import descriptor, mix, render

LONG = 10301  # samples of the long timeline: 40 chunks and 61 samples, so that a stateless master's render is cut into time segments


def clip(x):
    c = d.Clip(0.8)
    c.IN = d.Multiply(x, 1.7)
    return c


def lowpass(x):
    return d.Filter(x, 1200)


def comb(x):
    u = d.CombFilter(100 / 48000, 0.6)
    u.IN = x
    return u


def allpass(x):
    u = d.AllPass(113 / 48000, 0.5)
    u.IN = x
    return u


def _echo(x, delay=300.25):
    s = d.Sum(x, 0)
    dl = d.Delay(s, delay, 2048)
    s.B = d.Multiply(dl, 0.5)
    return s, dl


def echo(x):
    return _echo(x)[0]


def echo_at_delay(x):
    return _echo(x)[1]


def echo_of(delay):
    """the echo with a delay of its own: a master per channel (300.25 samples left, 411.5 right)"""
    return lambda x: _echo(x, delay)[0]


def reconvergent(x, delay=480):
    return d.Sum(x, d.Multiply(d.Delay(x, delay, 2048), 0.3))


def reconvergent_two_chunks_late(x):
    """what the reference's ONE circuit makes of `reconvergent` behind a Sum chain: its process order ticks the master's Multiply before
    its Delay and the Delay before the chain's last Sum, so each hears its source's previous chunk: the delayed path is 2 x 256 samples late"""
    return reconvergent(x, 480 + 2 * 256)


# name -> (fx, is the master over the stream the reference's one circuit fx(Sum.many(...)) bit for bit, on a mono piece?)
MASTERS = {"clip": (clip, True), "filter": (lowpass, True), "comb": (comb, True), "allpass": (allpass, True), "echo": (echo, True), "echo_at_delay": (echo_at_delay, True),
           "reconvergent": (reconvergent, False)}
# ... and on a piece of two channels, for those tried (the reference's comb family gives ONE channel for a two-channel input)
STEREO_MASTERS = {"filter": True, "echo": True, "comb": False}


def stereo_voice(k):
    """a two-channel voice that ends: mix_voices' panned triangle under the score voice's Ramp"""
    return d.Multiply(mix_voices.voice("pan", k), d.Ramp(700, 1, 0).trigger())


def unified_master(master, channels):
    d.configure(sv.SAMPLE_RATE)
    return render.master_program(master, channels, sv.SAMPLE_RATE)


def oracle_master(oracle, master, raw):
    """the oracle's render of `master` (a function, or a list of one a channel) over the raw timeline [channels, n_total]"""
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    uni = unified_master(master, raw.shape[0])
    return mix.master_chain(raw, lambda c, x: oracle.render(uni.words, raw.shape[1], params=uni.params, n_instances=raw.shape[0], instance=c, inputs=x[None])[0])


def words_of(outlet):
    d.configure(sv.SAMPLE_RATE)
    return descriptor.extract(outlet).words
