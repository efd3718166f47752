"""The limiter's release of its own on the device (dusp_limit_release_device, dusp_limit_release_host,
dusp_render_host_score_piece_limiter_release).  The envelope kernel and the three kernels behind it are held BIT FOR BIT
to the contract, mix.limit(..., release=R) fed the library's own taps and the same threshold: everything between the envelope's division
and the curve's division is integer, and the scan over the tiles is exact in (min, +) — there is nothing to bound.  Compared: the words
q, the held curve, the curve g, every limited sample and the reduction, with W what dusp_limit_release_tile reports.

The call: limiter=True, limiter_release=0.05 follows mix.deliver_limited(..., release=R) as tests/test_gpu_limiter.py follows it without a
release: given the threshold and the level the call reports, the limited signals, their true peaks, the reduction and every byte of the
frames are the model's exactly."""
import ctypes
import math

import numpy as np
import pytest

import dusp_amd as d
import meter_cases as mtc
from dusp_amd import mix, render, runtime, wav
from test_gpu_limiter import GUARD, ONE, RATE, SENTINEL32, T, WINDOW, bits32, bits64, library_taps, meters_dict, one_step, piece, reference, signals

pytestmark = pytest.mark.gpu

R_MAX = 1 << 22


def on_device(torch, ctx, x, rate, threshold, L, R, skip):
    """dusp_limit_release_device over x placed `skip` floats behind a 16-byte boundary, every buffer between fences ->
    (limited [S, C, n], q [n], held [n + L - 1], g [n], the smallest sum)"""
    S, C, n = x.shape
    fence = np.full(GUARD, SENTINEL32, dtype=np.uint32).view(np.float32)
    d_x = torch.from_numpy(np.concatenate([fence, np.zeros(skip, np.float32), x.ravel(), fence])).cuda()
    d_q = torch.from_numpy(np.full(GUARD + n + GUARD, SENTINEL32, dtype=np.uint32).view(np.int32)).cuda()
    d_h = torch.from_numpy(np.full(GUARD + n + L - 1 + GUARD, SENTINEL32, dtype=np.uint32).view(np.int32)).cuda()
    d_g = torch.from_numpy(np.full(GUARD + n + GUARD, -7.0)).cuda()
    d_w = torch.from_numpy(np.full(3, -7, dtype=np.int64)).cuda()
    ctx.limit_release_device(d_x.data_ptr() + 4 * (GUARD + skip), S, C, n, rate, threshold, L, R, d_q.data_ptr() + 4 * GUARD, d_h.data_ptr() + 4 * GUARD, d_g.data_ptr() + 8 * GUARD,
                             d_w.data_ptr() + 8, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.limit_release_last_ms()  # (waits for the call and checks the guards behind the context's scratch: q, and the held curve and the summaries)
    y, q, h, g, w = d_x.cpu().numpy(), d_q.cpu().numpy().view(np.uint32), d_h.cpu().numpy().view(np.uint32), d_g.cpu().numpy(), d_w.cpu().numpy()
    assert (y[:GUARD].view(np.uint32) == SENTINEL32).all() and (y[GUARD + skip + S * C * n:].view(np.uint32) == SENTINEL32).all() and not y[GUARD:GUARD + skip].any(), "wrote outside the signals"
    assert (q[:GUARD] == SENTINEL32).all() and (q[GUARD + n:] == SENTINEL32).all() and (h[:GUARD] == SENTINEL32).all() and (h[GUARD + n + L - 1:] == SENTINEL32).all(), "wrote outside q or held"
    assert (g[:GUARD] == -7.0).all() and (g[GUARD + n:] == -7.0).all() and w[0] == -7 and w[2] == -7, "wrote outside g or the word"
    return y[GUARD + skip:GUARD + skip + S * C * n].reshape(S, C, n), q[GUARD:GUARD + n], h[GUARD:GUARD + n + L - 1], g[GUARD:GUARD + n], int(w[1])


def held_to(torch, ctx, x, rate, threshold, L, R, taps, label, e=None, skips=(0, 1)):
    """two runs, on and off a 16-byte boundary, give the model's bits -> (limited, g, reduction)"""
    e = mix.limiter_envelope(x, rate, taps) if e is None else e
    g_want, q_want, h_want = mix.limiter_gain_release(e, threshold, L, R)
    with np.errstate(all="ignore"):
        want = (x.astype(np.float64) * g_want).astype(np.float32)
    reduction = float(g_want.min())
    for skip in skips:
        y, q, h, g, smallest = on_device(torch, ctx, x, rate, threshold, L, R, skip)
        assert np.array_equal(q, q_want), (label, skip, "q", np.flatnonzero(q != q_want)[:8])
        assert np.array_equal(h.astype(np.int64), h_want), (label, skip, "held", np.flatnonzero(h != h_want)[:8])
        assert np.array_equal(bits64(g), bits64(g_want)), (label, skip, "g", np.flatnonzero(g != g_want)[:8])
        assert np.array_equal(bits32(y), bits32(want)), (label, skip, "samples")
        assert smallest / float(L * ONE) == reduction, (label, skip, smallest, reduction)
    return want, g_want, reduction


@pytest.mark.parametrize("L", [1, 3, 64, 513])
def test_the_release_kernels_are_the_contract_bit_for_bit(L):
    """n = 1, 5, W - 1, W, W + 1, 2 W + 3 and 9 W + 7; R = 1, 2, L, W - 1, W, W + 1, 3 W + 1 and 2^22; one row and three signals of two
    channels, on and off a 16-byte boundary; F = 4, and 2 and 1 at two lengths; R = 1 is the plain limiter's curve"""
    import torch
    ctx = runtime.Context(-1, 48000)
    try:
        W = ctx.limit_release_tile(1000, L, 2400)
        assert W == 256 == ctx.limit_tile(1000, L)  # (a short call: a position a lane)
        limits = 0
        for rate in (48000, 96000, 192000):
            taps = library_taps(rate)
            for n in (1, 5, W - 1, W, W + 1, 2 * W + 3, 9 * W + 7) if rate == 48000 else (5, 2 * W + 3):
                for shape in ((1, 1), (3, 2)):
                    x = signals("noise", shape, n)
                    e = mix.limiter_envelope(x, rate, taps)
                    plain = mix.limiter_gain(e, T, L)[0]
                    for R in (1, 2, L, W - 1, W, W + 1, 3 * W + 1, R_MAX):
                        if shape == (3, 2) and R not in (1, W + 1, R_MAX) and n != 2 * W + 3:
                            continue  # (the rows change the envelope and the apply alone: every R at one length)
                        _, g, reduction = held_to(torch, ctx, x, rate, T, L, R, taps, (rate, L, n, shape, R), e)
                        limits += reduction < 1.0
                        assert (g <= plain).all() and (R > 1 or np.array_equal(bits64(g), bits64(plain)))
        assert limits > 60
        envelope_ms, hold_ms, release_ms, apply_ms = ctx.limit_release_last_ms()
        assert ctx.score_last_ms()[0] > 0 and envelope_ms > 0 and hold_ms > 0 and release_ms > 0 and apply_ms > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("L", [1, 3, 64, 513])
def test_peaks_at_the_tiles_edges_and_a_release_across_tiles(L):
    """a lone peak on a tile's first and last sample and L - 1 and L samples either side of the edge, the release short and long; a peak
    whose release crosses more than three tiles with a shallower and a deeper peak inside it and tiles that are all ONE in between; a
    NaN and an Inf; a threshold above everything"""
    import torch
    rate = 48000
    taps = library_taps(rate)
    ctx = runtime.Context(-1, 48000)
    try:
        W = ctx.limit_release_tile(1000, L, 2400)
        n = 2 * W + 3
        edges = {0, n - 1, W - 1, W, W - 1 - (L - 1), W - 1 - L, W + (L - 1), W + L, 2 * W - L, 2 * W + L - 1}
        for at in sorted(a for a in edges if 0 <= a < n):
            x = signals("lone", (3, 2), n, at, L)
            for R in (7, W + 1, 1 << 20):
                y, g, reduction = held_to(torch, ctx, x, rate, T, L, R, taps, (L, "lone", at, R), skips=(at & 1,))
                assert reduction < 0.21 and np.abs(y).max() <= T * (1 + 2.0 ** -23), "the peak of 2.5 or 3 comes out at T"
                if R == 1 << 20 and at + L + 40 < n:
                    assert (g[at + 20:] < 0.22).all(), "a release of twenty seconds has not let go within the call"
        # quiet noise, q = ONE everywhere but three peaks: a deep one, a shallower one inside its release, and a deeper one that takes over
        n = 9 * W + 7
        x = signals("quiet", (1, 1), n)
        x[0, 0, W // 2], x[0, 0, W + 40], x[0, 0, 6 * W + 5] = 40.0, 0.9, -90.0  # (q = ONE / 80, about 0.55 ONE, ONE / 180)
        e = mix.limiter_envelope(x, rate, taps)
        for R in (5 * W, 1 << 16):
            step = mix.limiter_release_step(R)
            y, g, reduction = held_to(torch, ctx, x, rate, T, L, R, taps, (L, "across", R), e)
            _, q, held = mix.limiter_gain_release(e, T, L, R)
            lone = x.copy()
            lone[0, 0, W + 40] = 0.0
            assert q[W + 40] < ONE and np.array_equal(held[W + 200:], mix.limiter_gain_release(mix.limiter_envelope(lone, rate, taps), T, L, R)[2][W + 200:]), "the shallower peak is under the release"
            # (from ONE / 80 a release of 5 W takes 79 / 80 x 5 W = 1264 positions, from position W / 2 + L - 1 on: past 4 W + L)
            rising = held[W + 300 + L:min(4 * W + L, 6 * W - 100)]  # (... and in front of the third peak's own minima)
            assert (q[W + 300:6 * W - 100] == ONE).all() and (rising < ONE).all() and (np.diff(rising) == step).all() and len(rising) > W, "tiles of ONE, crossed by the release"
            assert g[6 * W + 5] == reduction < 0.006 < g[6 * W - 2 * L - 40], "the deeper peak takes over"
        for kind in ("nan", "inf"):
            x = signals(kind, (3, 2), W + 1)
            y, _, _ = held_to(torch, ctx, x, rate, T, L, 700, taps, (L, kind))
            assert np.array_equal(np.isfinite(y), np.isfinite(x)) and np.isnan(y[2, 0, (W + 1) // 2]) == (kind == "nan")
        x = signals("quiet", (3, 2), 2 * W + 3)
        for R in (1, 2400, R_MAX):
            y, _, reduction = held_to(torch, ctx, x, rate, T, L, R, taps, (L, "quiet", R))
            assert reduction == 1.0 and np.array_equal(bits32(y), bits32(x)), "nothing over the threshold: bit for bit the input"
    finally:
        ctx.close()


def test_a_long_call_has_tiles_of_2048_and_the_host_round_trip_gives_the_same_bits():
    import torch
    rate = 48000
    taps = library_taps(rate)
    ctx = runtime.Context(-1, 48000)
    try:
        n, L, R = 2100001, 240, 24000
        assert ctx.limit_release_tile(n, L, R) == 2048
        x = signals("noise", (1, 1), n)
        x[0, 0, 5000:900000] *= 0.05  # (a long stretch under the threshold: the release of the last peak in front of it runs out in it)
        _, g, reduction = held_to(torch, ctx, x, rate, T, L, R, taps, "long", skips=(1,))
        assert reduction < 1.0 and (g[5000 + R + 2 * L:899000] == 1.0).all() and (g[5000 + L:5000 + R // 4] < 1.0).all()
        x = signals("noise", (3, 2), 777)
        for release in (1, 300, R_MAX):
            want, g_want, reduction = mix.limit(x, rate, T, 40, taps, release)
            for got in (ctx.limit(x, rate, T, 40, release), render.limit(x, rate, T, 40, release)):
                assert np.array_equal(bits32(got[0]), bits32(want)) and np.array_equal(bits64(got[1]), bits64(g_want)) and got[2] == reduction
        plain = mix.limit(x, rate, T, 40, taps)
        for got in (ctx.limit(x, rate, T, 40), ctx.limit(x, rate, T, 40, 0), render.limit(x, rate, T, 40), render.limit(x, rate, T, 40, None)):
            assert np.array_equal(bits32(got[0]), bits32(plain[0])) and np.array_equal(bits64(got[1]), bits64(plain[1])) and got[2] == plain[2], "without a release: the limiter as it was"
    finally:
        ctx.close()


def test_every_refusal_of_the_release_entries():
    import torch
    ctx = runtime.Context(-1, 48000)
    L = ctx._L
    x = np.zeros((2, 1, 400), dtype=np.float32)
    d_x, d_w = torch.from_numpy(x.ravel()).cuda(), torch.zeros(4, dtype=torch.int64, device="cuda")
    out = np.zeros_like(x)
    T_, W_ = ctypes.c_double(0.5), 40

    def refused(rc, *words):
        message = L.dusp_last_error(ctx._h).decode()
        assert rc != 0 and all(w in message for w in words), (rc, message)

    try:
        device = lambda planar, S, C, n, rate, t, w, r, q=None, h=None, g=None, word=None: L.dusp_limit_release_device(ctx._h, planar, S, C, n, rate, t, w, r, q, h, g, word, None)
        ms = (ctypes.c_float * 4)()
        refused(L.dusp_limit_release_last_ms(ctx._h, ctypes.addressof(ms)), "no dusp_limit_release_device call")
        refused(device(d_x.data_ptr(), 2, 1, 400, 0, T_, W_, 100), "dusp_limit_release_device", "needs a sample rate, not 0")
        refused(device(None, 2, 1, 400, 8000, T_, W_, 100), "dusp_limit_release_device: NULL buffer")
        refused(device(d_x.data_ptr(), 2, 1, 0, 8000, T_, W_, 100), "1..2^31 samples")
        refused(device(d_x.data_ptr(), 2, 1, 400, 8000, ctypes.c_double(math.nan), W_, 100), "threshold must be a finite number above 0")
        for bad in (0, 4097):
            refused(device(d_x.data_ptr(), 2, 1, 400, 8000, T_, bad, 100), "window is 1 .. 4096 samples, not %d" % bad)
        for bad in (0, R_MAX + 1):
            refused(device(d_x.data_ptr(), 2, 1, 400, 8000, T_, W_, bad), "dusp_limit_release_device", "release is 1 .. 4194304 samples, not %d" % bad)
            refused(L.dusp_limit_release_host(ctx._h, x.ctypes.data, 2, 1, 400, 8000, T_, W_, bad, out.ctypes.data, None, None), "dusp_limit_release_host", "not %d" % bad)
            assert L.dusp_limit_release_tile(ctx._h, 400, 40, bad) == 0
        refused(device(d_x.data_ptr(), 2, 1, 400, 8000, T_, W_, 100, None, d_w.data_ptr() + 2), "d_held must be 4-byte aligned")
        refused(device(d_x.data_ptr(), 2, 1, 400, 8000, T_, W_, 100, None, None, d_w.data_ptr() + 4), "8-byte aligned")
        refused(L.dusp_limit_release_host(ctx._h, None, 2, 1, 400, 8000, T_, W_, 100, out.ctypes.data, None, None), "dusp_limit_release_host: NULL buffer")
        assert L.dusp_limit_release_host(ctx._h, x.ctypes.data, 2, 1, 400, 8000, T_, W_, 100, out.ctypes.data, None, None) == 0 and not out.any()
        assert L.dusp_limit_release_tile(ctx._h, 400, 0, 100) == 0 and L.dusp_limit_release_tile(ctx._h, 0, 40, 100) == 0 and L.dusp_limit_release_tile(ctx._h, 400, 40, 100) == 256
        for release in (-1, R_MAX + 1, 2.5, True):
            with pytest.raises(ValueError) as e:  # (Context.limit refuses by string what the library would refuse)
                ctx.limit(x, 8000, 1.0, 40, release)
            assert str(e.value) == mix.LIMITER_RELEASE_SAMPLES
    finally:
        ctx.close()


# ---- the call -----------------------------------------------------------------------------------------------------------------------------

RELEASE = 400  # 50 ms at 8 kHz


@pytest.mark.parametrize("depth", [16, 24])
def test_a_delivery_with_a_release_where_the_limiter_engages(depth, capsys):
    ref, stack = reference()
    taps = library_taps(RATE)
    got = piece(d.render_piece_pcm, depth, 0, loudness=0, true_peak_max=-1.0, limiter=True, limiter_release=0.05)
    lim = got.limiter
    assert isinstance(got, render.Stems) and isinstance(lim, render.Limiter) and got.names == ref.names
    assert lim.engaged is True and lim.window == WINDOW and lim.release == RELEASE == mix.check_limiter_release(0.05, True, RATE)
    tp_in = np.stack([ref.meters.true_peak[k] for k in ref.names])
    assert bits64(lim.lufs_in) == bits64(ref.meters.lufs["mix"]) and lim.true_peak_in == tp_in.max()
    want_T = mix.limiter_threshold(lim.lufs_in, 0.0, -1.0)
    assert abs(lim.threshold - want_T) <= np.spacing(want_T) and lim.true_peak_in > lim.threshold
    # the limited signals, by the model at that threshold
    limited, g, reduction = mix.limit(stack, RATE, lim.threshold, WINDOW, taps, RELEASE)
    g_plain = mix.limit(stack, RATE, lim.threshold, WINDOW, taps)[1]
    assert lim.reduction == reduction < 1.0 and (g <= g_plain).all() and (g < g_plain).any()
    tp = np.stack([got.meters.true_peak[k] for k in got.names])
    assert np.array_equal(bits64(tp), bits64(mix.true_peak(limited, RATE, taps))), "the true peaks are the limited signals'"
    mtc.held("limited", meters_dict(got.meters), mix.meters(limited, RATE), limited, RATE)
    lufs = got.meters.lufs["mix"]
    gain, level = mix.loudness_gain(lufs, tp, 0.0, -1.0)
    assert isinstance(got.level, np.float32) and one_step(got.level, level) and got.gain == 1.0 / float(np.float64(got.level))
    frames, peaks = wav.encode_at_level(limited, depth, got.level)
    for k, name in enumerate(got.names):
        assert got[name].data.tobytes() == frames[k].tobytes(), name
        assert np.float32(got[name].peak).view(np.uint32) == peaks[k].view(np.uint32), "the peak is the limited signal's"
    model = mix.deliver_limited(stack, RATE, 0.0, -1.0, WINDOW, taps, RELEASE)
    assert model["limiter"]["engaged"] and model["limiter"]["release"] == RELEASE and abs(model["limiter"]["threshold"] / lim.threshold - 1) < 1e-9
    assert abs(model["limiter"]["reduction"] / lim.reduction - 1) < 1e-9 and abs(model["gain"] / got.gain - 1) < 1e-6
    # against the limiter without a release: the ceiling is held either way, and the release has taken loudness from the mix
    plain = piece(d.render_piece_pcm, depth, 0, loudness=0, true_peak_max=-1.0, limiter=True)
    ceiling = 10 ** (-1 / 20)
    with capsys.disabled():
        print("\nlimiter with a release of %d samples at %d bits: reduction %.6f; gain %.6f (without a release %.6f); delivered %.3f LUFS (without %.3f)"
              % (RELEASE, depth, lim.reduction, got.gain, plain.gain, lufs + 20 * math.log10(got.gain), plain.meters.lufs["mix"] + 20 * math.log10(plain.gain)))
    assert plain.limiter.release == 0 and tp.max() * got.gain <= ceiling * (1 + 2.0 ** -23) and lufs <= plain.meters.lufs["mix"]
    files = piece(d.render_piece_wav, depth, 0, loudness=0, true_peak_max=-1.0, limiter=True, limiter_release=0.05)
    assert files.level == got.level and files.gain == got.gain and files.mix == wav.encode_wav(got.mix.data, RATE, depth) and files.limiter.release == RELEASE


def test_the_piece_entry_without_a_release_not_engaged_and_refused(monkeypatch):
    # not engaged: the delivery is the one without a limiter, byte for byte
    quiet = piece(d.render_piece_pcm, 16, 0, loudness=-23, limiter=True, limiter_release=0.5)
    plain = piece(d.render_piece_pcm, 16, 0, loudness=-23)
    assert quiet.limiter.engaged is False and quiet.limiter.release == 4000 and quiet.gain == plain.gain
    for name in plain.names:
        assert quiet[name].data.tobytes() == plain[name].data.tobytes()
    # release_samples = 0 in the record: the entry without a release, byte for byte
    real = runtime.ScoreLimiterRelease
    was = piece(d.render_piece_pcm, 16, 0, loudness=0, limiter=True)
    monkeypatch.setattr(runtime, "ScoreLimiterRelease", lambda record, release: real(record, 0))
    through = piece(d.render_piece_pcm, 16, 0, loudness=0, limiter=True, limiter_release=0.05)
    assert through.limiter.engaged and through.limiter.reduction == was.limiter.reduction and through.gain == was.gain and through.level == was.level
    for name in was.names:
        assert through[name].data.tobytes() == was[name].data.tobytes(), name
    # more than 2^22 samples, behind the limiter entry's own refusals
    monkeypatch.setattr(runtime, "ScoreLimiterRelease", lambda record, release: real(record, R_MAX + 1))
    with pytest.raises(runtime.DuspHipError) as e:
        piece(d.render_piece_pcm, 16, 0, loudness=0, limiter=True, limiter_release=0.05)
    assert "dusp_render_host_score_piece_limiter_release" in str(e.value) and "release is 1 .. 4194304 samples, not %d" % (R_MAX + 1) in str(e.value), str(e.value)
    real_limiter = runtime.ScoreLimiter
    monkeypatch.setattr(runtime, "ScoreLimiter", lambda w, *where: real_limiter(4097, *where))
    with pytest.raises(runtime.DuspHipError, match="window is 1 .. 4096 samples, not 4097"):
        piece(d.render_piece_pcm, 16, 0, loudness=0, limiter=True, limiter_release=0.05)
    monkeypatch.undo()
    again = piece(d.render_piece_pcm, 16, 0, loudness=0, limiter=True, limiter_release=0.05)
    assert again.limiter.engaged and again.limiter.release == RELEASE, "a refused call leaves the next one whole"
    # render_score_pcm takes the keyword too
    d.configure(RATE)
    try:
        voices = [d.Multiply(d.Osc(200 + 50 * k), 0.8) for k in range(3)]
        base = d.render_score(voices, [0, 800, 1600], 0.5, 1.0, true_peak=True)
        got = d.render_score_pcm(voices, [0, 800, 1600], 0.5, 1.0, 16, 0, loudness=0, limiter=True, limiter_window=0.002, limiter_release=0.1)
    finally:
        d.configure(48000)
    x = np.stack(base.mix)[None]
    assert got.limiter.engaged and got.limiter.window == 16 and got.limiter.release == 800
    limited, _, reduction = mix.limit(x, RATE, got.limiter.threshold, 16, library_taps(RATE), 800)
    assert got.limiter.reduction == reduction and got.mix.data.tobytes() == wav.encode_at_level(limited, 16, got.level)[0][0].tobytes()
