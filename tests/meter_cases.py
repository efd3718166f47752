"""What the meter tests share (tests/test_meters_host.py, tests/test_gpu_meters.py, tests/test_js_meters.py): the signals they
use — the gated noise, noise on a DC offset, a planted Inf — and the bounds a cut of the K-weighting in time is held to against the
one sequential loop (mix.k_weighted), worked out from the coefficients and the number format, never from what the device gives."""
import functools
import math

import numpy as np

from dusp_amd import mix


def gated_noise(n=32123, shape=(1, 1), seed=1, rate=8000):
    """seeded normal noise x 0.1, float32 [S, C, n]; second 1 .. 2 x 0.001 (below the absolute gate), the half second behind it zero — at
    n = 32123, 8 kHz: samples 8000 .. 16000 and 16000 .. 20000.  The formulas give 37 blocks and -18.41 LUFS for the default."""
    x = (np.random.default_rng(seed).standard_normal(shape + (n,)) * 0.1).astype(np.float32)
    x[..., rate:2 * rate] *= np.float32(0.001)
    x[..., 2 * rate:2 * rate + rate // 2] = 0
    return x


def shaped_noise(n, shape, seed=2):
    """the same three stretches at any length: the second quarter x 0.001, the eighth behind it zero"""
    x = (np.random.default_rng(seed).standard_normal(shape + (n,)) * 0.1).astype(np.float32)
    x[..., n // 4:n // 2] *= np.float32(0.001)
    x[..., n // 2:n // 2 + n // 8] = 0
    return x


def dc_noise(n, shape, seed=3):
    """noise x 0.1 on a DC offset of 0.5: the RLB numerator (1, -2, 1) cancels the offset, the worst case for a scan over segments"""
    return (np.random.default_rng(seed).standard_normal(shape + (n,)) * 0.1 + 0.5).astype(np.float32)


def planted_inf(n, shape, seed=4):
    """noise with +Inf in the last channel of the last signal, a little behind the middle -> (signals, the sample)"""
    x = (np.random.default_rng(seed).standard_normal(shape + (n,)) * 0.1).astype(np.float32)
    at = min(n - 1, n // 2 + 3)
    x[-1, -1, at] = np.inf
    return x, at


def section_gain(a1, a2):
    """N = sum |g_k| over the impulse response of 1 / (1 + a1 z^-1 + a2 z^-2), added until it stops growing"""
    g1 = g2 = total = 0.0
    k = 0
    while True:
        g = (1.0 if k == 0 else 0.0) - a1 * g1 - a2 * g2
        grown = total + abs(g)
        if k > 16 and grown == total:
            return total
        total, g2, g1, k = grown, g1, g, k + 1


@functools.lru_cache(maxsize=None)
def gains(rate):
    shelf, rlb = mix.k_weighting(rate)
    return section_gain(shelf[3], shelf[4]), section_gain(rlb[3], rlb[4])


def sample_bound(rate, peak):
    """delta: what a sample of z may differ by between two roundings of the same linear recurrence — 2 x 8 operations a sample x 2^-53,
    through both sections' gains, on input up to `peak` (the largest finite magnitude)"""
    n_shelf, n_rlb = gains(rate)
    return 2.0 * 8.0 * 2.0 ** -53 * n_shelf * n_rlb * float(peak)


def energy_bound(e, channels, delta):
    """what a block energy e (the sum over `channels` of mean z^2) may differ by when every sample of z differs by at most delta"""
    return 2.0 * np.sqrt(channels * np.asarray(e, dtype=np.float64)) * delta + channels * delta * delta


def finite_peak(x):
    x = np.asarray(x, dtype=np.float64)
    x = np.abs(x[np.isfinite(x)])
    return float(x.max()) if x.size else 0.0


def held(name, got, want, signals, rate, report=None):
    """got: dict(rms, momentary, lufs) of a call, want: mix.meters(signals, rate) — every figure within its derived bound -> the largest
    observed ratio of an energy's difference to its bound.  rms^2 against math.fsum: all terms are non-negative, so any order is within
    n 2^-52 relative.  momentary and lufs: 10 log10(1 + rho), rho the largest relative energy bound over the blocks above the gates,
    + 1e-12 for log10 itself."""
    S, C, n = signals.shape
    delta, worst = sample_bound(rate, finite_peak(signals)), 0.0
    for s in range(S):
        for c in range(C):
            exact = math.fsum(float(v) * float(v) for v in signals[s, c].astype(np.float64)) / n
            ms = float(got["rms"][s][c]) ** 2
            if math.isfinite(exact):
                assert abs(ms - exact) <= (n + 4) * 2.0 ** -52 * exact, (name, s, c, ms, exact)
            else:
                assert not math.isfinite(ms), (name, s, c, ms)
        e = want["energies"][s]
        fine = np.isfinite(e)
        m_got, m_want = np.asarray(got["momentary"][s]), want["momentary"][s]
        assert m_got.shape == m_want.shape, (name, m_got.shape, m_want.shape)
        assert np.array_equal(np.isfinite(10.0 ** (m_got / 10)) | (m_got == -np.inf), fine), (name, s, "the blocks that are not finite")
        with np.errstate(all="ignore"):
            e_got = 10.0 ** ((m_got - mix.LUFS_OFFSET) / 10.0)
            bound = energy_bound(e, C, delta)
            # (e_got went through log10 and back: 1e-12 relative on top of the bound)
            ratio = np.where(fine & (bound > 0), np.abs(e_got - e) / (bound + 1e-12 * e), 0.0)
        if fine.any():
            worst = max(worst, float(ratio[fine].max()))
            assert ratio[fine].max() <= 1.0, (name, s, int(np.argmax(ratio)), float(ratio.max()))
        lufs = float(got["lufs"][s])
        if not fine.all():
            assert math.isnan(lufs) and math.isnan(want["lufs"][s]), (name, s, lufs)
            continue
        gated = fine & (m_want > mix.LUFS_ABSOLUTE_GATE)
        if not gated.any():
            assert lufs == -math.inf == want["lufs"][s], (name, s, lufs)
            continue
        rho = float((bound[gated] / e[gated]).max())
        tol = 10.0 * math.log10(1.0 + rho) + 1e-12
        assert abs(lufs - want["lufs"][s]) <= tol, (name, s, lufs, want["lufs"][s], tol)
        assert np.all(np.abs(m_got[gated] - m_want[gated]) <= tol), (name, s)
    if report is not None:
        report.append((name, worst))
    return worst
