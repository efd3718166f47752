"""The limiter's release of its own on the host: dusp_amd/mix.py limiter_release_step, limiter_gain_release, limit and
deliver_limited with release=, check_limiter_release — the contract's properties without a tolerance, curves checked by hand, a plain-Python
model of the tiled form the kernels use against the sequential recurrence, the refusals by string and the routing; and the text of the
release's kernels on the host under sanitizers (tests/native/limiter_release_kernel_check.cpp).  Needs no GPU."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import score_voices as sv
from dusp_amd import mix, render, runtime
from test_piece_host import ROOT, SANITIZE

ONE = 1 << 30
PLAIN = 192000  # F = 1: the envelope is |x|, largest over the rows
WINDOWS = (1, 3, 5, 64, 240, 4096)
RELEASES = (1, 7, 1000, 4096, 20000, 100000)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def envelopes():
    """test_limiter_host.py's signals: noise over and under the threshold, at three thresholds"""
    rng = np.random.default_rng(5)
    for T in (0.9, 1e-3, 37.5):
        yield T, np.abs(rng.standard_normal(700)) * rng.choice([0.01, 1.0, 90.0], 700) * T


def minima(q, L):
    """m[j + (L - 1)] = min(q[j .. j + L - 1]), q = ONE outside: the plain double loop"""
    n = len(q)
    a = [ONE] * (L - 1) + [int(v) for v in q] + [ONE] * (L - 1)
    return [min(a[i:i + L]) for i in range(n + L - 1)]


def recurrence(m, step):
    """held[j] = min(m[j], held[j - 1] + d), held[-L] = ONE, one position after the other in Python's integers"""
    held, last = [], ONE
    for v in m:
        last = min(int(v), last + step)
        held.append(last)
    return held


def test_the_step():
    assert mix.LIMITER_RELEASE_MAX == 1 << 22
    assert mix.limiter_release_step(1) == ONE and mix.limiter_release_step(16) == 1 << 26 and mix.limiter_release_step(3) == 357913942 and mix.limiter_release_step(1 << 22) == 256
    for R in (1, 2, 7, 1000, 4095, 48000, (1 << 22) - 1, 1 << 22):
        step = mix.limiter_release_step(R)
        assert step == -(-ONE // R) and step * R >= ONE > step * (R - 1) - R and -(-ONE // step) <= R, "a gain of 0 is back at 1 after at most R samples"
    for bad in (0, -1, (1 << 22) + 1, 2.5, True):
        with pytest.raises(ValueError) as e:
            mix.limiter_release_step(bad)
        assert str(e.value) == mix.LIMITER_RELEASE_SAMPLES


def test_the_four_properties_hold_exactly():
    """(1) R = 1 is limiter_gain's curve bit for bit; (2) held <= m, so g_release <= g_plain <= r; (3) held rises by at most d a position
    and the sum by at most L d a sample; (4) held[j] depends on the last ceil(ONE / d) <= R values of m alone — all without a tolerance."""
    for T, e in envelopes():
        r = np.where(e > T, T / np.where(e > T, e, 1.0), 1.0)
        for L in WINDOWS:
            plain, q_plain = mix.limiter_gain(e, T, L)
            m = np.array(minima(q_plain, L), dtype=np.int64)
            g1, q1, held1 = mix.limiter_gain_release(e, T, L, 1)
            assert np.array_equal(g1, plain) and np.array_equal(q1, q_plain) and np.array_equal(held1, m) and g1.dtype == np.float64 and q1.dtype == np.uint32
            for R in RELEASES:
                step = mix.limiter_release_step(R)
                g, q, held = mix.limiter_gain_release(e, T, L, R)
                assert held.shape == (len(e) + L - 1,) and held.dtype == np.int64 and np.array_equal(q, q_plain)
                assert held.tolist() == recurrence(m, step), (T, L, R)
                assert (held <= m).all() and (held >= 0).all() and (g <= plain).all() and (plain <= r).all() and (g > 0).all()
                assert (np.diff(np.concatenate(([ONE], held))) <= step).all()
                sums = np.rint(g * float(L * ONE)).astype(np.int64)  # (below 2^43: exact in f64)
                assert np.array_equal(sums, np.convolve(held, np.ones(L, dtype=np.int64), "valid")) and (np.diff(sums) <= L * step).all()
                back = -(-ONE // step)
                assert back <= R
                for j in (0, 1, len(m) // 2, len(m) - 1):  # the closed form over the bounded look-back alone
                    lo = max(0, j - back + 1)
                    assert held[j] == min(ONE, min(int(m[i]) + step * (j - i) for i in range(lo, j + 1))), (T, L, R, j)
                if R >= 1000 and L < 4096:
                    assert (g < plain).any(), "a longer release holds the gain down longer"


def test_release_none_is_the_limiter_as_it_was():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((3, 2, 400)).astype(np.float32)
    for rate in (8000, 48000, PLAIN):
        for L in (1, 40):
            e = mix.limiter_envelope(x, rate)
            g_was, _ = mix.limiter_gain(e, 0.5, L)
            was = (x.astype(np.float64) * g_was).astype(np.float32)
            for release in (None, 1):
                limited, g, reduction = mix.limit(x, rate, 0.5, L) if release is None else mix.limit(x, rate, 0.5, L, release=release)
                assert np.array_equal(g, g_was) and reduction == g_was.min() and np.array_equal(bits32(limited), bits32(was))
            limited, g, reduction = mix.limit(x, rate, 0.5, L, None, None)
            assert np.array_equal(g, g_was)
            slow = mix.limit(x, rate, 0.5, L, release=5000)
            assert (slow[1] <= g_was).all() and (slow[1] < g_was).any() and slow[2] <= reduction
    # a threshold above everything: every bit stays, whatever the release
    top = mix.limiter_envelope(x, 48000).max()
    limited, g, reduction = mix.limit(x, 48000, top, 64, release=48000)
    assert (g == 1.0).all() and reduction == 1.0 and np.array_equal(bits32(limited), bits32(x))


def curve(held, n, L):
    return np.array([sum(held[s:s + L]) for s in range(n)], dtype=np.float64) / float(L * ONE)


def test_curves_checked_by_hand():
    half, quarter = ONE // 2, ONE // 4
    # L = 1: held is the recurrence over q itself, g = held / ONE
    e = np.array([0.5, 4.0, 1.0, 1.0, 1.0, 2.0, 1.0])
    g, q, held = mix.limiter_gain_release(e, 1.0, 1, 4)  # d = ONE / 4
    assert held.tolist() == [ONE, quarter, half, 3 * quarter, ONE, half, 3 * quarter] and np.array_equal(g, [1.0, 0.25, 0.5, 0.75, 1.0, 0.5, 0.75])
    # a lone peak of q = ONE / 2, L = 4, R = 16: d = 2^26, the four minima that see the peak, then back at ONE after 8 steps
    n, p = 41, 20
    e = np.full(n, 0.25)
    e[p] = 2.0
    g, q, held = mix.limiter_gain_release(e, 1.0, 4, 16)
    step = 1 << 26
    assert mix.limiter_release_step(16) == step and q[p] == half and half + 8 * step == ONE
    want = [ONE] * (n + 3)  # position j + 3 holds held[j]
    for j in range(p - 3, p + 1):
        want[j + 3] = half
    for k in range(1, 8):
        want[p + k + 3] = half + k * step
    assert held.tolist() == want and held[p + 8 + 3] == ONE and held[p + 7 + 3] == ONE - step
    assert np.array_equal(g, curve(want, n, 4)) and g[p] == 0.5 and g[p - 4] == 1.0 and g[p - 3] == 7 / 8 and g[p - 1] == 5 / 8, "the attack is the plain limiter's"
    assert g[p + 1] == (3 * half + half + step) / (4.0 * ONE) and g[p + 8 + 3] == 1.0 and g[p + 8 + 2] == (4 * ONE - step) / (4.0 * ONE) and (np.diff(g[p:]) >= 0).all()
    # the peak at sample 0 and at sample n - 1: the release runs from the peak, or there is no room for it
    for p in (0, n - 1):
        e = np.full(n, 0.25)
        e[p] = 4.0
        g, q, held = mix.limiter_gain_release(e, 1.0, 8, 32)  # d = ONE / 32: 24 steps back up from a quarter
        want = [ONE] * (n + 7)
        for j in range(p - 7, p + 1):
            want[j + 7] = quarter
        for k in range(1, 24):
            if p + k + 7 < n + 7:
                want[p + k + 7] = quarter + k * (ONE // 32)
        assert held.tolist() == want and np.array_equal(g, curve(want, n, 8)) and g[p] == 0.25
    # R > n: the curve never comes back within the signal
    e = np.full(10, 0.25)
    e[2] = 8.0
    g, q, held = mix.limiter_gain_release(e, 1.0, 2, 1000)
    step = mix.limiter_release_step(1000)
    # (position j + 1 holds held[j]; the minima at j = 1 and 2 see the peak)
    assert held.tolist() == [ONE, ONE, ONE // 8, ONE // 8] + [ONE // 8 + k * step for k in range(1, 8)] and g[9] == (2 * (ONE // 8) + 13 * step) / (2.0 * ONE) and (g[2:] < 0.14).all()
    # a shallower peak inside a deeper one's release does not show in held; a deeper one takes over
    e = np.full(40, 0.25)
    e[5], e[9], e[20] = 8.0, 1.25, 16.0
    g, q, held = mix.limiter_gain_release(e, 1.0, 1, 64)  # d = ONE / 64
    step = ONE // 64
    lone = np.full(40, 0.25)
    lone[5], lone[20] = 8.0, 16.0
    assert q[9] == math.floor(ONE / 1.25) > ONE // 8 + 4 * step and np.array_equal(held, mix.limiter_gain_release(lone, 1.0, 1, 64)[2]), "the shallower peak is under the release"
    assert held[9] == ONE // 8 + 4 * step and held[19] == ONE // 8 + 14 * step and held[20] == ONE // 16 and held[21] == ONE // 16 + step and np.array_equal(g, held / float(ONE))


def tiled(m, step, W):
    """The kernels' form in plain Python: a summary a tile, the carry from at most ceil(ONE / (d W)) + 1 summaries back, and inside the
    tile the prefix minimum of m[i] + d (W - 1 - i) — no negative number, everything below 2^43"""
    positions = len(m)
    tiles = -(-positions // W)
    at = lambda j: int(m[j]) if j < positions else ONE
    summary = [min(ONE, min(at(b * W + i) + step * (W - 1 - i) for i in range(W))) for b in range(tiles)]
    look_back = -(-ONE // (step * W)) + 1
    held, most = [], 0
    for b in range(tiles):
        carry = ONE
        for k in range(1, min(b, look_back) + 1):
            reach = summary[b - k] + step * W * (k - 1)
            most = max(most, reach)
            carry = min(carry, reach)
        running = None
        for i in range(W):
            if b * W + i >= positions:
                break
            v = at(b * W + i) + step * (W - 1 - i)
            running = v if running is None else min(running, v)
            most = max(most, running, carry + step * (i + 1))
            held.append(min(running - step * (W - 1 - i), carry + step * (i + 1)))
    assert most < 1 << 43
    return held, summary


def test_the_tiled_form_is_the_recurrence():
    rng = np.random.default_rng(11)
    n = 4500
    noise = np.where(rng.random(n) < 0.02, rng.integers(0, ONE + 1, n), ONE)
    sparse = np.full(n, ONE)  # a deep dip whose release spans more than three tiles, a shallower and a deeper one inside it, tiles all ONE
    sparse[300], sparse[900], sparse[2500] = 5, ONE // 2, 1
    sparse[4400] = ONE // 3
    for W in (256, 333, 1024):
        for q in (noise, sparse, np.full(n, ONE)):
            for L in (1, 64, 240):
                m = minima(q, L)
                for R in (1, 7, W, 3 * W + 1, 4096, 100000, 1 << 22):
                    step = mix.limiter_release_step(R)
                    got, summary = tiled(m, step, W)
                    assert got == recurrence(m, step), (W, L, R)
                    if q is sparse and R >= 100000 and W < 1024:
                        assert summary.count(ONE) >= 3 and got[2400] < ONE, "the release of the dip at 300 crosses tiles whose own summary is ONE (more than three of 256 or 333)"
                    if q is sparse and R == 7:
                        assert summary.count(ONE) >= 3, "tiles that are all ONE in between"
    # the release of 4 W: the carry of a tile comes from a summary three tiles back through two tiles that are all ONE
    W, R = 256, 1024
    q = np.full(5 * W, ONE)
    q[10] = 0
    step = mix.limiter_release_step(R)
    got, summary = tiled(minima(q, 1), step, W)
    assert summary[1] == ONE == summary[2] and got == recurrence(q, step) and got[3 * W] == step * (3 * W - 10) < ONE


def test_the_whole_chain_of_a_delivery_with_a_release():
    rng = np.random.default_rng(19)
    n = 8000
    x = (0.05 * rng.standard_normal((2, 1, n))).astype(np.float32)
    x[:, 0, 5000] = 0.9
    x[1] = x[0]
    plain = mix.deliver_limited(x, 8000, -16.0, -1.0, 40)
    assert plain["limiter"]["release"] == 0
    out = mix.deliver_limited(x, 8000, -16.0, -1.0, 40, release=800)
    lim = out["limiter"]
    assert lim["engaged"] and lim["release"] == 800 and lim["window"] == 40 and lim["threshold"] == plain["limiter"]["threshold"] and lim["lufs_in"] == plain["limiter"]["lufs_in"]
    limited, g, reduction = mix.limit(x, 8000, lim["threshold"], 40, release=800)
    assert lim["reduction"] == reduction == plain["limiter"]["reduction"] and np.array_equal(bits32(out["signals"]), bits32(limited))
    assert (g <= mix.limit(x, 8000, lim["threshold"], 40)[1]).all()
    gain, level = mix.loudness_gain(mix.meters(limited, 8000)["lufs"][-1], mix.true_peak(limited, 8000), -16.0, -1.0)
    assert (out["gain"], out["level"]) == (gain, level)
    assert out["true_peak"].max() * gain <= 10 ** (-1 / 20) * (1 + 2.0 ** -23), "the ceiling is held by the static gain"
    assert out["meters"]["lufs"][-1] <= plain["meters"]["lufs"][-1], "a longer release takes more loudness from the mix"
    quiet = mix.deliver_limited(x, 8000, -40.0, -1.0, 40, release=800)
    assert not quiet["limiter"]["engaged"] and quiet["limiter"]["release"] == 800 and np.array_equal(bits32(quiet["signals"]), bits32(x))


# ---- the refusals and the routing ---------------------------------------------------------------------------------------------------------

def test_check_limiter_release():
    assert mix.check_limiter_release(None, False, 48000) == 0 and mix.check_limiter_release(None, "unread", 48000) == 0
    assert mix.check_limiter_release(0.05, True, 48000) == 2400 and mix.check_limiter_release(0.5, np.bool_(True), 44100) == 22050 and mix.check_limiter_release(1e-9, True, 8000) == 1
    assert mix.check_limiter_release((1 << 22) / 48000, True, 48000) == 1 << 22 and mix.check_limiter_release(np.float32(0.25), True, 96000) == 24000 and mix.check_limiter_release(1, True, 8000) == 8000
    for value in (0, -0.05, math.nan, math.inf, "50ms", True, False):
        for limiter in (True, False):
            with pytest.raises(ValueError) as e:
                mix.check_limiter_release(value, limiter, 48000)
            assert str(e.value) == mix.LIMITER_RELEASE_BAD
    for limiter in (False, np.bool_(False)):
        with pytest.raises(ValueError) as e:
            mix.check_limiter_release(0.05, limiter, 48000)
        assert str(e.value) == mix.LIMITER_RELEASE_NEEDS_LIMITER
    with pytest.raises(ValueError) as e:
        mix.check_limiter_release(100.0, True, 48000)
    assert str(e.value) == mix.LIMITER_RELEASE_LONG % (4800000, 48000) and "4800000 samples at 48000 Hz" in str(e.value)
    with pytest.raises(ValueError) as e:
        mix.check_limiter_release(((1 << 22) + 1) / 48000, True, 48000)
    assert str(e.value) == mix.LIMITER_RELEASE_LONG % ((1 << 22) + 1, 48000)
    for huge in (1e300, 1.7e308):
        with pytest.raises(ValueError) as e:
            mix.check_limiter_release(huge, True, 48000)
        assert str(e.value) == mix.LIMITER_RELEASE_LONG % (2 ** 62, 48000)
    for bad in (0, (1 << 22) + 1, 2.5):
        with pytest.raises(ValueError) as e:
            mix.limiter_gain_release(np.ones(4), 1.0, 2, bad)
        assert str(e.value) == mix.LIMITER_RELEASE_SAMPLES


CALLS = (d.render_piece, d.render_score, d.render_piece_pcm, d.render_score_pcm, d.render_piece_wav, d.render_score_wav)
PCM_CALLS = CALLS[2:]


def voices(n=3):
    d.configure(sv.SAMPLE_RATE)
    return [sv.voice(k) for k in range(n)]


@pytest.mark.parametrize("call", PCM_CALLS, ids=lambda f: f.__name__)
def test_what_a_release_does_not_go_with_is_refused_by_string(call):
    with pytest.raises(ValueError) as e:
        call(voices(), [0, 1, 2], 0.01, 0.05, 16, 0, loudness=-16, limiter_release=0.05)
    assert str(e.value) == mix.LIMITER_RELEASE_NEEDS_LIMITER
    with pytest.raises(ValueError) as e:
        call(voices(), [0, 1, 2], 0.01, 0.05, 16, 0, limiter_release=0.05)
    assert str(e.value) == mix.LIMITER_RELEASE_NEEDS_LIMITER
    for value in (0, -1, math.nan, math.inf, "50ms", True):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, 16, 0, loudness=-16, limiter=True, limiter_release=value)
        assert str(e.value) == mix.LIMITER_RELEASE_BAD
    with pytest.raises(ValueError) as e:
        call(voices(), [0, 1, 2], 0.01, 0.05, 16, 0, loudness=-16, limiter=True, limiter_release=1000.0)
    assert str(e.value) == mix.LIMITER_RELEASE_LONG % (1000 * sv.SAMPLE_RATE, sv.SAMPLE_RATE)
    with pytest.raises(ValueError) as e:
        call(voices(), [0, 1, 2], 0.01, 0.05, 16, 0, loudness=-16, limiter=True, limiter_window=1.0, limiter_release=1000.0)
    assert str(e.value) == mix.LIMITER_WINDOW_LONG % (sv.SAMPLE_RATE, sv.SAMPLE_RATE)  # (the window's refusals come first)
    with pytest.raises(ValueError) as e:
        call(voices(), [0, 1, 2], 0.01, 0.05, 16, 0, limiter=True, limiter_release=0.05)
    assert str(e.value) == mix.LIMITER_NEEDS_LOUDNESS


def test_a_release_on_the_planar_calls_is_refused_as_loudness_is():
    for call in (d.render_piece, d.render_score):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, loudness=-16, limiter=True, limiter_release=0.05)
        assert str(e.value) == mix.LOUDNESS_PLANAR
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, limiter=True, limiter_release=0.05)
        assert str(e.value) == mix.LIMITER_NEEDS_LOUDNESS
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, limiter_release=0.05)
        assert str(e.value) == mix.LIMITER_RELEASE_NEEDS_LIMITER


def test_the_keyword_travels_with_the_placement_and_the_record_reports_it():
    d.configure(sv.SAMPLE_RATE)
    plain = render._placing(None, None, None, None, -3, None, False)
    assert plain["limiter_release"] is None
    placing = render._placing(None, None, None, None, -3, None, False, loudness=-16, limiter=True, limiter_window=0.002, limiter_release=0.05)
    *_, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, placing)
    assert place.limiter is True and place.limiter_release == 0.05 and "limiter_release" not in place.keywords()
    # a timeline of no samples renders nothing: the record has the release in samples, and 0 without one
    release = mix.check_limiter_release(0.05, True, sv.SAMPLE_RATE)
    one = d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 0, loudness=-16, limiter=True, limiter_release=0.05)
    assert isinstance(one.limiter, render.Limiter) and (one.limiter.engaged, one.limiter.release, one.limiter.reduction) == (False, release, 1.0) and release == round(0.05 * sv.SAMPLE_RATE)
    none = d.render_score_wav(voices(), [0, 1, 2], 0.01, 0, 16, 0, loudness=-16, limiter=True)
    assert none.limiter.release == 0 and none.limiter.window == mix.check_limiter(True, 0.005, -16, sv.SAMPLE_RATE)
    assert render.Limiter(dict(engaged=1, threshold=0.5, window=3, reduction=0.25, lufs_in=-20.0, true_peak_in=1.0)).release == 0
    # the library has the entries (they are detected by symbol), and their refusals
    L = runtime.load()
    for name in ("dusp_limit_release_tile", "dusp_limit_release_device", "dusp_limit_release_last_ms", "dusp_limit_release_host", "dusp_render_host_score_piece_limiter_release"):
        assert hasattr(L, name), name
    assert L.dusp_limit_release_tile(None, 1000, 240, 2400) == 0


# ---- the kernels' text, under sanitizers ------------------------------------------------------------------------------------------------

def test_limiter_release_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/limiter_release_engine.hip itself, compiled for the host — the lanes of a workgroup as threads, LDS as statics,
    __syncthreads a barrier (tests/native/hip_host_stub_lds; the shuffles and the 64-bit atomicMin in the program itself) — every buffer
    a heap allocation of exactly its size, under AddressSanitizer and UBSan, bit for bit against the plain loops
    (tests/native/limiter_release_kernel_check.cpp lists what it covers).  A stand-alone program, run as a subprocess; nothing is loaded
    into Python under a sanitizer."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "limiter_release_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub_lds"), "-x", "c++",
                           os.path.join(native, "limiter_release_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 250 and rep["groups"] > 2000 and rep["per_lane"] == 1 | 2 | 4 | 8, rep
