"""The deep-timeline model (tests/deep_time.py) pinned to the CPU oracle: windows of the model equal the oracle's sequential render bit
for bit — at shallow depth for every voice set and sample rate the GPU tests use, and once across sample 2^24 for a voice of each kind.
No GPU."""
import numpy as np
import pytest

import deep_time as dt
import deep_time_cases as dc
import edge_values as ev

SHALLOW_FIRST = (0, 2048, 1 << 20)
WINDOW_N = (2048, 2048 + 256 * 3 + 37)


@pytest.mark.parametrize("sr", dc.RATES)
@pytest.mark.parametrize("kind,env", dc.SETS)
def test_model_windows_equal_the_oracle_at_shallow_depth(kind, env, sr, oracle):
    vs = dc.voices(kind, env, sr)
    words, osc_units = dc.chain(vs, sr)
    n_total = max(SHALLOW_FIRST) + max(WINDOW_N)
    want, states = oracle.render(words, n_total, max_channels=1, return_state=True)
    for first in SHALLOW_FIRST:
        for n in WINDOW_N:
            got = dt.chain_window(vs, sr, first, n)
            assert ev.same_bits(got, want[0, first:first + n]), (kind, env, sr, first, n)
    # a chain cut after its third voice: the raw partial sum handed on as `init`
    first, n = 2048, WINDOW_N[1]
    part = dt.chain_window(vs[:3], sr, first, n, raw=True)
    assert ev.same_bits(dt.chain_window(vs[3:], sr, first, n, init=part), want[0, first:first + n])
    for v, u in zip(vs, osc_units):
        assert states[u][0] == dt.end_phase(v[1], sr, dt.whole_chunks(n_total)), (v, sr)


DEEP_N = (1 << 24) + 4099
DEEP_VOICES = [("osc", dc.f32(12345.678)), ("gain", 440.5, 0.625), ("ramp", -3.25, ((1 << 24) + 1000, 1, 0))]  # (the Ramp ends inside the tail)


@pytest.mark.parametrize("voice", DEEP_VOICES, ids=[v[0] for v in DEEP_VOICES])
def test_model_windows_equal_the_oracle_across_two_to_the_24(voice, oracle):
    sr = 48000
    words, osc_units = dc.chain([voice], sr)
    want, states = oracle.render(words, DEEP_N, max_channels=1, return_state=True)
    for first, n in ((0, 4096), ((1 << 24) - 2048, 4096), (DEEP_N - 4099, 4099)):
        assert ev.same_bits(ev.outlet(dt.voice_window(voice, sr, first, n)), want[0, first:first + n]), (voice, first)
    assert states[osc_units[0]][0] == dt.end_phase(voice[1], sr, dt.whole_chunks(DEEP_N))
