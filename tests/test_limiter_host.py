"""The look-ahead true-peak limiter without a device: the contract — mix.limiter_envelope, mix.limiter_gain and
mix.limit on curves that can be checked by hand, the property g <= r held EXACTLY, what a threshold at or above everything, a tiny
threshold, a NaN and an Inf do, the residual true peak of limited signals, the stems that still add up under one curve — the refusal
strings and the routing of limiter= and limiter_window=, the library's limiter_threshold against Python's, and the text of the
limiter's kernels on the host under sanitizers (tests/native/limiter_kernel_check.cpp)."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
from dusp_amd import mix, render, runtime
from test_piece_host import ROOT, SANITIZE

ONE = 1 << 30
PLAIN = 192000  # F = 1: the envelope is |x|, largest over the rows


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the curve --------------------------------------------------------------------------------------------------------------------------

def test_the_constants_and_the_envelope_are_the_true_peaks_own():
    assert mix.LIMITER_ONE == ONE and mix.LIMITER_WINDOW_MAX == 4096
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 2, 500)).astype(np.float32)
    assert np.array_equal(mix.limiter_envelope(x, PLAIN), np.abs(x.astype(np.float64)).max(axis=(0, 1)))
    for rate, D in ((48000, 6), (96000, 12)):
        # a lone unit sample: phase 0's centre tap is 1, so the envelope at that very sample is exactly 1 — the delay D is compensated
        impulse = np.zeros((1, 1, 60), dtype=np.float32)
        impulse[0, 0, 30] = 1.0
        e = mix.limiter_envelope(impulse, rate)
        assert e[30] == 1.0 and np.argmax(e) == 30 and e.shape == (60,) and (e[:30 - D] == 0).all()
        # every envelope value is one of true_peak's accumulators: the largest of them is the true peak unless the head or tail holds it
        assert mix.limiter_envelope(x, rate).max() == mix.true_peak(x, rate).max()
    assert mix.limiter_envelope(np.zeros((2, 1, 0), np.float32), 48000).shape == (0,)
    with pytest.raises(ValueError, match="shape \\(signals, channels, samples\\)"):
        mix.limiter_envelope(np.zeros((2, 5), np.float32), 48000)


def test_the_gain_is_at_most_r_exactly():
    """g[s] <= r[s] at every sample, as f64 numbers with no tolerance: every minimum in the mean of g[s] holds q[s], and floor and the
    integer mean only round down.  And no lower than the smallest r within the window less one unit of the fixed point: g[s] is a mean of
    minima over samples |j - s| < L.  (g[s] <= r[j] for EVERY |j - s| < L does not follow from the definition: the minimum that begins
    at s does not see s - 1.)"""
    rng = np.random.default_rng(5)
    for L in (1, 2, 3, 7, 64, 333, 1000):
        for T in (0.9, 1e-3, 37.5):
            e = np.abs(rng.standard_normal(700)) * rng.choice([0.01, 1.0, 90.0], 700) * T
            g, q = mix.limiter_gain(e, T, L)
            r = np.where(e > T, T / np.where(e > T, e, 1.0), 1.0)
            assert g.dtype == np.float64 and q.dtype == np.uint32 and np.array_equal(q, np.floor(r * ONE).astype(np.uint32)) and q.max() <= ONE
            assert (g <= r).all() and (g > 0).all() and (g <= 1.0).all() and (g < 1.0).any(), (L, T)
            padded = np.concatenate([np.ones(L - 1), r, np.ones(L - 1)])
            around = np.lib.stride_tricks.sliding_window_view(padded, 2 * L - 1).min(axis=1)  # min r[s - L + 1 .. s + L - 1]
            assert (g >= around - 2.0 ** -30).all(), (L, T)


def test_a_threshold_at_or_above_everything_leaves_every_bit():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((3, 2, 400)).astype(np.float32)
    x[1, 0, 17] = -0.0
    for rate in (8000, 96000, PLAIN):
        top = mix.limiter_envelope(x, rate).max()
        for T in (top, 2 * top, 1e300):
            for L in (1, 40, 4096):
                limited, g, reduction = mix.limit(x, rate, T, L)
                assert (g == 1.0).all() and reduction == 1.0 and limited.dtype == np.float32 and np.array_equal(bits32(limited), bits32(x))
        assert mix.limit(x, rate, np.nextafter(top, 0), 3)[2] < 1.0  # (one step below the top: the limiter works)


def ramp(n, p, L, depth_q):
    """the curve of ONE sample p whose q is depth_q, all others ONE, by hand: sum[s] = L ONE - c (ONE - depth_q) with c = L - |s - p| the
    minima of the window that see p, as an exact fraction of L ONE"""
    c = np.clip(L - np.abs(np.arange(n) - p), 0, None)
    return (L * ONE - c * (ONE - depth_q)).astype(np.float64) / float(L * ONE)


def test_curves_checked_by_hand():
    # L = 1: no window at all, g = floor(r ONE) / ONE
    e = np.array([0.5, 3.0, 1.0, 7.0, 1.0000001])
    g, q = mix.limiter_gain(e, 1.0, 1)
    assert np.array_equal(q, [ONE, math.floor(ONE / 3.0), ONE, math.floor(ONE / 7.0), math.floor(1.0 / 1.0000001 * ONE)]) and np.array_equal(g, q / float(ONE))
    # a single peak of twice the threshold in the middle: a linear attack of L samples, a linear release of L samples, exact fractions
    n, p = 41, 20
    e = np.full(n, 0.25)
    e[p] = 2.0
    for L in (4, 5):
        g, q = mix.limiter_gain(e, 1.0, L)
        assert q[p] == ONE // 2 and (np.delete(q, p) == ONE).all() and np.array_equal(g, ramp(n, p, L, ONE // 2))
        assert g[p] == 0.5 and g[p - L] == 1.0 == g[p + L] and g[p - L + 1] == (2 * L - 1) / (2 * L) == g[p + L - 1]
        assert np.array_equal(g[p - L:p + 1], np.arange(2 * L, L - 1, -1) / (2.0 * L)) and np.array_equal(g[p - L:p + L + 1], g[p - L:p + L + 1][::-1]), "linear and symmetric"
    assert np.array_equal(mix.limiter_gain(e, 1.0, 5)[0][p - 5:p + 6], [1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0])
    # the peak at sample 0 and at sample n - 1: half a ramp; outside [0, n) q is ONE, so nothing else pulls the curve down
    for p in (0, n - 1):
        e = np.full(n, 0.25)
        e[p] = 4.0
        g, _ = mix.limiter_gain(e, 1.0, 8)
        assert np.array_equal(g, ramp(n, p, 8, ONE // 4)) and g[p] == 0.25 and g[abs(p - 8)] == 1.0
    # L > n: the window is longer than the signal, and the curve is the same formula on what there is of it
    e = np.array([0.25, 0.25, 8.0, 0.25, 0.25])
    g, _ = mix.limiter_gain(e, 1.0, 100)
    assert np.array_equal(g, ramp(5, 2, 100, ONE // 8)) and g[2] == 0.125 and g[0] == (100 * 8 - 98 * 7) / 800
    # two peaks nearer than L: the minimum holds the deeper one, the mean blends
    e = np.full(30, 0.25)
    e[10], e[12] = 2.0, 4.0
    g, _ = mix.limiter_gain(e, 1.0, 3)
    half, quarter = ONE // 2, ONE // 4  # m[8] = m[9] = half, m[10] = m[11] = m[12] = quarter, every other minimum ONE
    assert g[12] == 0.25 and g[10] == (half + half + quarter) / (3.0 * ONE) and g[11] == (half + quarter + quarter) / (3.0 * ONE) and g[13] == 0.5 and g[7] == 1.0 == g[15]
    for bad_T in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError) as err:
            mix.limiter_gain(e, bad_T, 3)
        assert str(err.value) == mix.LIMITER_THRESHOLD_BAD
    for bad_L in (0, 4097, 2.5, -3):
        with pytest.raises(ValueError) as err:
            mix.limiter_gain(e, 1.0, bad_L)
        assert str(err.value) == mix.LIMITER_WINDOW_SAMPLES


def test_a_tiny_threshold_drives_q_to_0_and_the_output_to_signed_zeros():
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((2, 1, 300)) + 3.0 * rng.choice([-1, 1], (2, 1, 300))).astype(np.float32)  # (no sample near 0)
    for T in (1e-300, 5e-324, 1e-12):
        limited, g, reduction = mix.limit(x, PLAIN, T, 16)
        _, q = mix.limiter_gain(mix.limiter_envelope(x, PLAIN), T, 16)
        assert (q == 0).all() and (g == 0.0).all() and reduction == 0.0
        assert not limited.any() and np.array_equal(np.signbit(limited), np.signbit(x)), "+-0, the sample's sign kept"


def test_a_nan_and_an_inf_are_ignored_by_the_envelope_and_kept_in_the_output():
    rng = np.random.default_rng(11)
    for rate in (48000, 96000, PLAIN):
        x = (0.3 * rng.standard_normal((2, 2, 200))).astype(np.float32)
        x[0, 1, 50] = 3.0
        dirty = x.copy()
        dirty[1, 0, 120], dirty[0, 0, 160] = np.nan, -np.inf
        e, e_dirty = mix.limiter_envelope(x, rate), mix.limiter_envelope(dirty, rate)
        assert np.isfinite(e_dirty).all() and (e_dirty <= e).all() and np.array_equal(e_dirty[:100], e[:100]), "an accumulator that is not finite counts as 0"
        limited, g, _ = mix.limit(dirty, rate, 0.5, 10)
        assert np.isfinite(g).all() and (g > 0).all() and np.isnan(limited[1, 0, 120]) and limited[0, 0, 160] == -np.inf
        assert np.isfinite(np.delete(limited.ravel(), [2 * 200 + 120, 160])).all() and abs(limited[0, 1, 50]) <= 0.5


# ---- what the limiter leaves above the threshold --------------------------------------------------------------------------------------------

def residual_signals():
    n, t = 6000, np.arange(6000)
    burst = 0.05 * np.sin(2 * np.pi * t / 37.0)
    burst[2800:3200] = 1.5
    impulse = 0.1 * np.sin(2 * np.pi * t / 23.0)
    impulse[3000] = 2.0
    loud_end = 0.1 * np.sin(2 * np.pi * t / 29.0)
    loud_end[-50:] *= 12.0
    made = dict(quarter=np.sin(2 * np.pi * t / 4.0 + np.pi / 4), square=0.9 * np.where((t // 24) % 2 == 0, 1.0, -1.0), noise=0.3 * np.random.default_rng(1).standard_normal(n), burst=burst,
                impulse=impulse, loud_end=loud_end)
    return {name: x.astype(np.float32)[None, None] for name, x in made.items()}


def test_the_residual_true_peak_of_limited_signals(capsys):
    """mix.true_peak(limited) <= 1.01 T for six signals of 6000 samples at 8, 44.1, 48 and 96 kHz, T at 0.9, 0.5 and 0.25 of the true
    peak, a 5 ms window (measured: at most 1.0057, at 8 kHz, on the noise); at 192 kHz (F = 1) the ratio stays within 2^-23 of 1.
    The residual comes from the curve's slope between the oversampled points and grows as the window gets shorter in samples.  The
    noise is numpy's default_rng(1); the 1 % is no property of every noise: over the seeds 0 .. 23 the worst ratio at 8 kHz (a window
    of 40 samples) lies between 1.0045 and 1.0120, at 48 kHz (240 samples) between 1.0002 and 1.0012."""
    worst = {}
    for rate in (8000, 44100, 48000, 96000, 192000):
        L = mix.check_limiter(True, 0.005, -16, rate)
        assert L == max(1, round(0.005 * rate))
        for name, x in residual_signals().items():
            tp = float(mix.true_peak(x, rate).max())
            for part in (0.9, 0.5, 0.25):
                T = part * tp
                limited, _, reduction = mix.limit(x, rate, T, L)
                ratio = float(mix.true_peak(limited, rate).max()) / T
                worst[rate] = max(worst.get(rate, 0.0), ratio)
                assert reduction < 1.0
                if rate == 192000:
                    assert abs(ratio - 1.0) <= 2.0 ** -23, (rate, name, part, ratio)
                else:
                    assert ratio <= 1.01, (rate, name, part, ratio)
    with capsys.disabled():
        print("\nresidual true peak over the threshold, the worst a rate: " + ", ".join("%d Hz %.6f" % (rate, w) for rate, w in sorted(worst.items())))


def test_the_stems_still_add_up_under_one_curve():
    """Three stems x_1..x_S and their left-deep f32 chain a_1 = x_1, a_k = fl(a_(k-1) + x_k) as the mix m = a_S, all limited under ONE
    curve g.  The limited stems are y_i = fl(g x_i) = g x_i (1 + d_i), |d_i| <= u = 2^-24.  Let A = |y_1| + .. + |y_S| at a sample, the
    magnitudes of the LIMITED stems — the largest partial sum of the magnitudes, which to first order in u is g (|x_1| + .. + |x_S|)
    and so bounds every term and every partial sum of the limited chain and g times those of the unlimited one.  The left-deep f32 sum
    b_S of the limited stems differs from the limited mix fl(g m) by
        sum_i g x_i d_i          (the S roundings of the limited stems: together at most u A)
      + sum_(k=2..S) eta_k       (the S - 1 roundings of the limited chain, each at most u |b_k| <= u A)
      - g sum_(k=2..S) eps_k     (the S - 1 roundings of the unlimited chain, each at most u |a_k|, times g: at most u A)
      - g m d_m                  (the rounding of the limited mix, at most u g |m| <= u A)
    which is at most (1 + (S - 1) + (S - 1) + 1) u A = 2 S 2^-24 A, to first order in u.  Measured: at most 0.56 of that bound, 1.6 x
    2^-24 of the peak, for S = 3."""
    rng = np.random.default_rng(17)
    S, n = 3, 5000
    stems = (rng.standard_normal((S, 2, n)) * np.array([0.9, 0.3, 0.6])[:, None, None]).astype(np.float32)
    stems[0, 0, 1234] = 4.0
    stack = np.concatenate([stems, mix.stems_sum(np.concatenate([stems, stems[:1]]))[None]])  # (the mix last: the f32 chain of the stems)
    assert np.array_equal(bits32(stack[-1]), bits32((stems[0] + stems[1]) + stems[2]))
    worst = 0.0
    for rate, L in ((48000, 240), (PLAIN, 7)):
        limited, g, reduction = mix.limit(stack, rate, 0.7, L)
        assert reduction < 0.5
        again = mix.stems_sum(limited)
        A = np.abs(limited[:-1].astype(np.float64)).sum(axis=0)  # (of the LIMITED stems)
        assert (A <= g * np.abs(stems.astype(np.float64)).sum(axis=0) * (1 + 2.0 ** -23)).all() and (g < 1.0).all()
        diff = np.abs(again.astype(np.float64) - limited[-1].astype(np.float64))
        assert (diff <= 2 * S * 2.0 ** -24 * A).all(), float((diff[A > 0] / A[A > 0]).max() * 2.0 ** 24)
        worst = max(worst, float(diff.max() / np.abs(limited[-1]).max() * 2.0 ** 24))
        assert not np.array_equal(bits32(again), bits32(limited[-1])), "to f32 roundings, no longer bit for bit"
    assert worst < 2 * S


def test_the_whole_chain_of_a_delivery():
    rng = np.random.default_rng(19)
    n = 8000
    x = (0.05 * rng.standard_normal((2, 1, n))).astype(np.float32)
    x[:, 0, 5000] = 0.9
    x[1] = x[0]
    out = mix.deliver_limited(x, 8000, -16.0, -1.0, 40)
    lim = out["limiter"]
    base = mix.meters(x, 8000)
    assert lim["engaged"] and lim["lufs_in"] == base["lufs"][-1] and lim["true_peak_in"] == mix.true_peak(x, 8000).max() and lim["window"] == 40
    assert lim["threshold"] == mix.limiter_threshold(base["lufs"][-1], -16.0, -1.0) < lim["true_peak_in"]
    limited, _, reduction = mix.limit(x, 8000, lim["threshold"], 40)
    assert lim["reduction"] == reduction and np.array_equal(bits32(out["signals"]), bits32(limited))
    gain, level = mix.loudness_gain(mix.meters(limited, 8000)["lufs"][-1], mix.true_peak(limited, 8000), -16.0, -1.0)
    assert (out["gain"], out["level"]) == (gain, level) and gain > mix.loudness_gain(base["lufs"][-1], mix.true_peak(x, 8000), -16.0, -1.0)[0]
    assert out["true_peak"].max() * gain <= 10 ** (-1 / 20) * (1 + 2.0 ** -23), "the ceiling is held by the static gain"
    # a target so low that nothing comes near the ceiling, and silence: not engaged, the delivery without a limiter
    for signals, target in ((x, -40.0), (np.zeros_like(x), -16.0)):
        out = mix.deliver_limited(signals, 8000, target, -1.0, 40)
        assert not out["limiter"]["engaged"] and out["limiter"]["reduction"] == 1.0 and out["signals"] is not None and np.array_equal(bits32(out["signals"]), bits32(signals))
        assert (out["gain"], out["level"]) == mix.loudness_gain(mix.meters(signals, 8000)["lufs"][-1], mix.true_peak(signals, 8000), target, -1.0)


# ---- the threshold, the refusals and the routing ----------------------------------------------------------------------------------------------

def test_the_librarys_threshold_is_pythons():
    L = runtime.load()
    for lufs, target, ceiling in ((-20.0, -16.0, -1.0), (-4.47, 0.0, -1.0), (-33.3, -14.0, -2.5), (-23.0, -23.0, 0.0), (-70.0, -9.0, -0.1), (-math.inf, -16.0, -1.0), (-20.0, 7000.0, -1.0),
                                  (-20.0, -7000.0, -1.0)):
        got, want = L.dusp_limiter_threshold(lufs, target, ceiling), mix.limiter_threshold(lufs, target, ceiling)
        assert got == want or abs(got - want) <= 2 * np.spacing(want), (lufs, target, ceiling, got, want)
    assert mix.limiter_threshold(-20.0, -16.0, -1.0) == 10 ** (-1 / 20) / 10 ** (4 / 20) and mix.limiter_threshold(-math.inf, -16.0, -1.0) == 0.0
    assert math.isnan(L.dusp_limiter_threshold(math.nan, -16.0, -1.0)) and math.isnan(mix.limiter_threshold(math.nan, -16.0, -1.0))


def test_check_limiter():
    assert mix.check_limiter(False, "anything", None, 48000) == 0 and mix.check_limiter(np.bool_(False), 0.005, -16, 48000) == 0
    assert mix.check_limiter(True, 0.005, -16, 48000) == 240 and mix.check_limiter(True, 0.005, -16.0, 44100) == 220 and mix.check_limiter(np.bool_(True), 0.005, -16, 8000) == 40
    assert mix.check_limiter(True, 1e-9, -16, 8000) == 1 and mix.check_limiter(True, 4096 / 48000, -16, 48000) == 4096 and mix.check_limiter(True, np.float32(0.01), 0, 96000) == 960
    for value in (1, 0, None, "on", 1.0):
        with pytest.raises(ValueError) as e:
            mix.check_limiter(value, 0.005, -16, 48000)
        assert str(e.value) == mix.LIMITER_NOT_BOOL
    with pytest.raises(ValueError) as e:
        mix.check_limiter(True, 0.005, None, 48000)
    assert str(e.value) == mix.LIMITER_NEEDS_LOUDNESS
    for value in (0, -0.005, math.nan, math.inf, "5ms", None, True):
        with pytest.raises(ValueError) as e:
            mix.check_limiter(True, value, -16, 48000)
        assert str(e.value) == mix.LIMITER_WINDOW_BAD
    with pytest.raises(ValueError) as e:
        mix.check_limiter(True, 0.1, -16, 48000)
    assert str(e.value) == mix.LIMITER_WINDOW_LONG % (4800, 48000)
    for huge in (1e300, 1.7e308):  # (the second overflows to inf once multiplied by the sample rate)
        with pytest.raises(ValueError) as e:
            mix.check_limiter(True, huge, -16, 48000)
        assert str(e.value) == mix.LIMITER_WINDOW_LONG % (2 ** 62, 48000)


CALLS = (d.render_piece, d.render_score, d.render_piece_pcm, d.render_score_pcm, d.render_piece_wav, d.render_score_wav)
PCM_CALLS = CALLS[2:]


def voices(n=3):
    d.configure(sv.SAMPLE_RATE)
    return [sv.voice(k) for k in range(n)]


@pytest.mark.parametrize("call", CALLS, ids=lambda f: f.__name__)
def test_a_limiter_that_is_no_bool_is_refused_by_string_next_to_true_peak(call):
    for value in (1, 0, None, "on", 2.0):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, limiter=value, pans=[0])  # (the pans' shape would be refused next)
        assert str(e.value) == mix.LIMITER_NOT_BOOL
    with pytest.raises(ValueError) as e:
        call(voices(), [0, 1, 2], 0.01, 0.05, limiter=1, true_peak=1)
    assert str(e.value) == mix.TRUE_PEAK_NOT_BOOL  # (true_peak first)


@pytest.mark.parametrize("call", PCM_CALLS, ids=lambda f: f.__name__)
def test_what_a_limiter_does_not_go_with_is_refused_by_string(call):
    with pytest.raises(ValueError) as e:
        call(voices(), [0, 1, 2], 0.01, 0.05, 16, 0, limiter=True)
    assert str(e.value) == mix.LIMITER_NEEDS_LOUDNESS
    for value in (0, -1, math.nan, math.inf, "5ms", None):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, 16, 0, loudness=-16, limiter=True, limiter_window=value)
        assert str(e.value) == mix.LIMITER_WINDOW_BAD
    with pytest.raises(ValueError) as e:
        call(voices(), [0, 1, 2], 0.01, 0.05, 16, 0, loudness=-16, limiter=True, limiter_window=1.0)
    assert str(e.value) == mix.LIMITER_WINDOW_LONG % (sv.SAMPLE_RATE, sv.SAMPLE_RATE)
    with pytest.raises(ValueError) as e:
        call(voices(), [0, 1, 2], 0.01, 0.05, 16, 2, loudness=-16, limiter=True)
    assert str(e.value) == mix.LOUDNESS_WITH_NORMALISE % 2  # (the refusals of loudness come first)


def test_a_limiter_on_the_planar_calls_is_refused_by_string():
    for call in (d.render_piece, d.render_score):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, limiter=True)
        assert str(e.value) == mix.LIMITER_NEEDS_LOUDNESS
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, loudness=-16, limiter=True)
        assert str(e.value) == mix.LOUDNESS_PLANAR  # (as loudness is refused there)


def test_the_new_keywords_travel_with_the_placement_to_the_piece_and_a_timeline_of_no_samples():
    d.configure(sv.SAMPLE_RATE)
    plain = render._placing(None, None, None, None, -3, None, False)
    assert plain["limiter"] is False and plain["limiter_window"] == 0.005
    placing = render._placing(None, None, None, None, -3, None, False, stems=True, loudness=-16, limiter=True, limiter_window=0.002)
    *_, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, placing)
    assert place.limiter is True and place.limiter_window == 0.002 and place.loudness == -16
    assert not {"limiter", "limiter_window"} & set(place.keywords())
    # a score with a limiter goes the piece's way, as one part
    with pytest.raises(d.DuspError, match="the voices of a score are isomorphic circuits"):
        d.render_score_pcm([sv.voice(0), mc.stereo_voice(1)], [0, 1], 0.01, 0, 16, 0, loudness=-16, limiter=True)
    # a timeline of no samples renders nothing: the limiter's record says so
    window = mix.check_limiter(True, 0.005, -16, sv.SAMPLE_RATE)
    one = d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 0, loudness=-16, limiter=True)
    assert isinstance(one, render.Metered) and isinstance(one.limiter, render.Limiter) and one.gain == 1.0
    assert (one.limiter.engaged, one.limiter.window, one.limiter.reduction, one.limiter.lufs_in, one.limiter.true_peak_in) == (False, window, 1.0, -math.inf, 0.0)
    with_tracks = dict(tracks=[mc.echo, None], track_of=[0, 1, -1], faders=[1, 0.5], buses=[mc.comb], track_sends=[[1, 0]])
    files = d.render_score_wav(voices(), [0, 1, 2], 0.01, 0, 16, 0, stems=True, loudness=-23, limiter=True, limiter_window=0.001, **with_tracks)
    assert isinstance(files, render.Stems) and files.limiter.engaged is False and files.limiter.window == mix.check_limiter(True, 0.001, -23, sv.SAMPLE_RATE) and files.mix[:4] == b"RIFF"
    # without the new keywords a call hands back what it did
    assert not hasattr(d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 0, loudness=-16), "limiter")
    assert not hasattr(d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 0, loudness=-16, limiter=False, limiter_window="unread"), "limiter")


# ---- the kernels' text, under sanitizers ------------------------------------------------------------------------------------------------

def test_limiter_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/limiter_engine.hip itself, compiled for the host — the lanes of a workgroup as threads, LDS as statics,
    __syncthreads a barrier (tests/native/hip_host_stub_lds; the shuffle and the 64-bit atomicMin in the program itself) — every buffer
    a heap allocation of exactly its size, under AddressSanitizer and UBSan, bit for bit against the contract's loops
    (tests/native/limiter_kernel_check.cpp lists what it covers).  A stand-alone program, run as a subprocess; nothing is loaded into
    Python under a sanitizer."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "limiter_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub_lds"), "-x", "c++",
                           os.path.join(native, "limiter_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 300 and rep["groups"] > 2000 and rep["per_lane"] == 1 | 2 | 4 | 8, rep
