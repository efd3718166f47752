"""The look-ahead true-peak limiter on the device (dusp_limit_device, dusp_limit_host, dusp_render_host_score_piece_limiter; DESIGN.md
6.20).  The two kernels are held BIT FOR BIT to the contract, mix.limit fed the library's own taps and the same threshold: the envelope
forms every product and sum in the contract's order, unfused, an unsigned maximum commutes, and everything between the envelope's
division and the curve's division is integer — there is nothing to bound.  Compared: the words q, the curve g, every limited sample and
the reduction.

The call: limiter=True follows the model's whole chain — meters, T, limit, meters, true peaks, loudness_gain.  What the library takes
from its OWN meters is compared as the meters are (tests/meter_cases.py held: the K-weighting is a recurrence whose order of rounding
the kernel may choose) and what it takes from pow to one step in the last place, as tests/test_gpu_loudness.py does; given the threshold and the level the
call reports, the limited signals, their true peaks, the reduction and every byte of the frames are the model's exactly."""
import ctypes
import functools
import math

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import meter_cases as mtc
from dusp_amd import descriptor, mix, render, runtime, wav

pytestmark = pytest.mark.gpu

SENTINEL32 = 0x5EA15EA1
GUARD = 16
ONE = 1 << 30
RATES = {8000: 4, 48000: 4, 96000: 2, 192000: 1}
T = 0.5


def library_taps(rate):
    factor, h49 = ctypes.c_int(0), (ctypes.c_double * 49)()
    assert runtime.load().dusp_true_peak_taps(rate, ctypes.byref(factor), h49) == 0
    return factor.value, np.array(h49[:] if factor.value > 1 else h49[:1])


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def signals(kind, shape, n, at=0, L=1):
    """noise: about a third of the samples over T; lone: quiet noise and ONE peak at sample `at`, in a row that moves with at and L;
    nan, inf: noise with one planted in the last signal; quiet: nothing near T"""
    S, C = shape
    rng = np.random.default_rng(n * 7 + S * 3 + C + len(kind) + at + L)
    x = ((0.05 if kind in ("lone", "quiet") else 0.5) * rng.standard_normal((S, C, n))).astype(np.float32)
    if kind == "lone":
        x.reshape(S * C, n)[(at + L) % (S * C), at] = -3.0 if at & 1 else 2.5
    elif kind in ("nan", "inf"):
        x[S - 1, 0, n // 2] = np.nan if kind == "nan" else -np.inf
    return x


def on_device(torch, ctx, x, rate, threshold, L, skip):
    """dusp_limit_device over x placed `skip` floats behind a 16-byte boundary, every buffer between fences ->
    (limited [S, C, n], q [n], g [n], the smallest sum)"""
    S, C, n = x.shape
    fence = np.full(GUARD, SENTINEL32, dtype=np.uint32).view(np.float32)
    d_x = torch.from_numpy(np.concatenate([fence, np.zeros(skip, np.float32), x.ravel(), fence])).cuda()
    d_q = torch.from_numpy(np.full(GUARD + n + GUARD, SENTINEL32, dtype=np.uint32).view(np.int32)).cuda()
    d_g = torch.from_numpy(np.full(GUARD + n + GUARD, -7.0)).cuda()
    d_w = torch.from_numpy(np.full(3, -7, dtype=np.int64)).cuda()
    ctx.limit_device(d_x.data_ptr() + 4 * (GUARD + skip), S, C, n, rate, threshold, L, d_q.data_ptr() + 4 * GUARD, d_g.data_ptr() + 8 * GUARD, d_w.data_ptr() + 8,
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.limit_last_ms()  # (waits for the call and checks the guard behind the context's scratch, which the envelope kernel writes q into)
    y, q, g, w = d_x.cpu().numpy(), d_q.cpu().numpy().view(np.uint32), d_g.cpu().numpy(), d_w.cpu().numpy()
    assert (y[:GUARD].view(np.uint32) == SENTINEL32).all() and (y[GUARD + skip + S * C * n:].view(np.uint32) == SENTINEL32).all() and not y[GUARD:GUARD + skip].any(), "wrote outside the signals"
    assert (q[:GUARD] == SENTINEL32).all() and (q[GUARD + n:] == SENTINEL32).all() and (g[:GUARD] == -7.0).all() and (g[GUARD + n:] == -7.0).all() and w[0] == -7 and w[2] == -7, "wrote outside q, g or the word"
    return y[GUARD + skip:GUARD + skip + S * C * n].reshape(S, C, n), q[GUARD:GUARD + n], g[GUARD:GUARD + n], int(w[1])


def held(torch, ctx, x, rate, threshold, L, taps, label):
    """two runs, on and off a 16-byte boundary, give the model's bits -> (limited, reduction)"""
    e = mix.limiter_envelope(x, rate, taps)
    g_want, q_want = mix.limiter_gain(e, threshold, L)
    want, g_again, reduction = mix.limit(x, rate, threshold, L, taps)
    assert np.array_equal(bits64(g_want), bits64(g_again))
    for skip in (0, 1):
        y, q, g, smallest = on_device(torch, ctx, x, rate, threshold, L, skip)
        assert np.array_equal(q, q_want), (label, skip, "q", np.flatnonzero(q != q_want)[:8])
        assert np.array_equal(bits64(g), bits64(g_want)), (label, skip, "g", np.flatnonzero(g != g_want)[:8])
        assert np.array_equal(bits32(y), bits32(want)), (label, skip, "samples")
        assert smallest / float(L * ONE) == reduction, (label, skip, smallest, reduction)
    return want, reduction


@pytest.mark.parametrize("rate", sorted(RATES))
def test_the_limiter_kernels_are_the_contract_bit_for_bit(rate):
    """n = 1, 5 and around the tile W; L = 1, 2, 3, 64 and 4096 — above n at the small n; one row, two rows of odd length (the second
    off a 16-byte boundary) and three signals of two channels; a lone peak at sample 0, n - 1, W - 1 and W and L - 1 and L samples on
    either side of the tile's edge, where a short halo shows, in a different row each time; a NaN and an Inf, which the envelope
    ignores and the output keeps; a threshold above everything leaves every bit and a reduction of exactly 1"""
    import torch
    taps = library_taps(rate)
    assert taps[0] == RATES[rate]
    ctx = runtime.Context(-1, 48000)
    try:
        W = ctx.limit_tile(1000, 64)
        assert W == 256 and ctx.limit_tile(1000, 4096) == 256  # (a short call: a sample a lane)
        limits = 0
        for L in (1, 2, 3, 64, 4096):
            for n in (1, 5, W - 1, W, W + 1, 2 * W + 3):
                for shape in [(1, 1), (3, 2)] + ([(1, 2)] if n % 2 else []):
                    _, reduction = held(torch, ctx, signals("noise", shape, n), rate, T, L, taps, (rate, L, n, shape, "noise"))
                    limits += reduction < 1.0
            n = 2 * W + 3
            edges = {0, n - 1, W - 1, W, W - 1 - (L - 1), W - 1 - L, W + (L - 1), W + L, 2 * W - L, 2 * W + L - 1}
            for at in sorted(a for a in edges if 0 <= a < n):
                x = signals("lone", (3, 2), n, at, L)
                y, reduction = held(torch, ctx, x, rate, T, L, taps, (rate, L, n, "lone", at))
                assert reduction < 0.21 and np.abs(y).max() <= T * (1 + 2.0 ** -23), "the peak of 2.5 or 3 comes out at T"
        assert limits > 40
        for L in (3, 64):
            for kind in ("nan", "inf"):
                x = signals(kind, (3, 2), W + 1)
                y, _ = held(torch, ctx, x, rate, T, L, taps, (rate, L, kind))
                assert np.array_equal(np.isfinite(y), np.isfinite(x)) and np.isnan(y[2, 0, (W + 1) // 2]) == (kind == "nan")
                clean = x.copy()
                clean[2, 0, (W + 1) // 2] = 0.0
                assert np.array_equal(mix.limiter_envelope(x, rate, taps)[(W + 1) // 2 + 30:], mix.limiter_envelope(clean, rate, taps)[(W + 1) // 2 + 30:])
            x = signals("quiet", (3, 2), 2 * W + 3)
            y, reduction = held(torch, ctx, x, rate, T, L, taps, (rate, L, "quiet"))
            assert reduction == 1.0 and np.array_equal(bits32(y), bits32(x)), "nothing over the threshold: bit for bit the input"
        k, _, _ = ctx.score_last_ms()
        envelope_ms, apply_ms = ctx.limit_last_ms()
        assert k > 0 and envelope_ms > 0 and apply_ms > 0
    finally:
        ctx.close()


def test_a_long_call_takes_more_samples_a_lane_and_the_host_round_trip_gives_the_same_bits():
    """enough samples that the grid rule gives a lane 2 and 8 samples, and 4 under a long window: whatever the tile, the contract's bits"""
    import torch
    rate = 48000
    taps = library_taps(rate)
    ctx = runtime.Context(-1, 48000)
    try:
        seen = set()
        for shape, n, L in (((1, 2), 600001, 64), ((1, 1), 2100001, 240), ((1, 1), 1100001, 600)):
            W = ctx.limit_tile(n, L)
            seen.add(W)
            x = signals("noise", shape, n)
            want, g_want, reduction = mix.limit(x, rate, T, L, taps)
            y, q, g, smallest = on_device(torch, ctx, x, rate, T, L, 1)
            assert np.array_equal(bits32(y), bits32(want)) and np.array_equal(bits64(g), bits64(g_want)) and smallest / float(L * ONE) == reduction < 1.0, (shape, n, L, W)
        assert seen == {512, 2048, 1024}, seen
        x = signals("noise", (3, 2), 777)
        want, g_want, reduction = mix.limit(x, rate, T, 40, taps)
        for got in (ctx.limit(x, rate, T, 40), render.limit(x, rate, T, 40)):
            assert np.array_equal(bits32(got[0]), bits32(want)) and np.array_equal(bits64(got[1]), bits64(g_want)) and got[2] == reduction
        one = render.limit(x[0], rate, T, 40)
        assert one[0].shape == (2, 777) and np.array_equal(bits32(one[0]), bits32(mix.limit(x[:1], rate, T, 40, taps)[0][0]))
    finally:
        ctx.close()


def test_every_refusal_of_the_limiter_entries():
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
        device = lambda planar, S, C, n, rate, t, w, q=None, g=None, word=None: L.dusp_limit_device(ctx._h, planar, S, C, n, rate, t, w, q, g, word, None)
        ms = (ctypes.c_float * 2)()
        refused(L.dusp_limit_last_ms(ctx._h, ctypes.addressof(ms)), "no dusp_limit_device call")
        refused(device(d_x.data_ptr(), 2, 1, 400, 0, T_, W_), "dusp_limit_device", "needs a sample rate, not 0")
        refused(device(None, 2, 1, 400, 8000, T_, W_), "dusp_limit_device: NULL buffer")
        refused(device(d_x.data_ptr(), 2, 0, 400, 8000, T_, W_), "1..64 channels")
        refused(device(d_x.data_ptr(), 2, 1, 0, 8000, T_, W_), "1..2^31 samples")
        for bad in (0.0, -1.0, math.nan, math.inf):
            refused(device(d_x.data_ptr(), 2, 1, 400, 8000, ctypes.c_double(bad), W_), "threshold must be a finite number above 0")
        for bad in (0, 4097):
            refused(device(d_x.data_ptr(), 2, 1, 400, 8000, T_, bad), "window is 1 .. 4096 samples, not %d" % bad)
        refused(device(d_x.data_ptr() + 2, 2, 1, 399, 8000, T_, W_), "4-byte aligned")
        refused(device(d_x.data_ptr(), 2, 1, 400, 8000, T_, W_, None, d_w.data_ptr() + 4), "8-byte aligned")
        refused(device(d_x.data_ptr(), 2, 1, 400, 8000, T_, W_, None, None, d_w.data_ptr() + 4), "8-byte aligned")
        refused(L.dusp_limit_host(ctx._h, None, 2, 1, 400, 8000, T_, W_, out.ctypes.data, None, None), "dusp_limit_host: NULL buffer")
        refused(L.dusp_limit_host(ctx._h, x.ctypes.data, 2, 1, 400, 8000, T_, W_, None, None, None), "dusp_limit_host: NULL buffer")
        refused(L.dusp_limit_host(ctx._h, x.ctypes.data, 2, 1, 400, 8000, T_, 4097, out.ctypes.data, None, None), "dusp_limit_host", "not 4097")
        assert L.dusp_limit_host(ctx._h, x.ctypes.data, 2, 1, 400, 8000, T_, W_, out.ctypes.data, None, None) == 0 and not out.any()  # (the curve and the reduction may be NULL)
        assert L.dusp_limit_tile(ctx._h, 400, 0) == 0 and L.dusp_limit_tile(ctx._h, 0, 40) == 0 and L.dusp_limit_tile(ctx._h, 400, 4097) == 0
        for threshold, window in ((0.0, 40), (math.nan, 40), (1.0, 0), (1.0, 4097), (1.0, 2.5)):
            with pytest.raises(ValueError) as e:  # (Context.limit refuses by string what the library would refuse)
                ctx.limit(x, 8000, threshold, window)
            assert str(e.value) == (mix.LIMITER_WINDOW_SAMPLES if threshold == 1.0 else mix.LIMITER_THRESHOLD_BAD)
    finally:
        ctx.close()


# ---- the call -----------------------------------------------------------------------------------------------------------------------------

RATE = 8000
NT = 8017  # about a second: two blocks and a last short hop at 8 kHz; odd, so that the second channel's rows start off a 16-byte boundary
N = 5
ONSETS = [0, 700, 1900, 2500, 3300]
PANS = [-0.6, 0.3, 0.0, 0.8, -0.2]
TRACK_OF = [0, 1, -1, 0, 1]
WINDOW = 40  # 5 ms at 8 kHz


def notes(scale):
    d.configure(RATE)
    return [d.Multiply(d.Osc(180.5 + 97 * k), scale * (0.5 + 0.1 * k)) for k in range(N)]


def piece(call=d.render_piece, *more, scale=0.4, stems=True, gains=None, **kw):
    """five notes of 4000 samples, panned, two tracks (a clip and a bare fader group), one bus fed by the tracks"""
    made = notes(scale)
    try:
        return call(made, ONSETS, 4000.5 / RATE, (NT + 0.5) / RATE, *more, lengths=None, gains=gains, pans=PANS, tracks=[mc.clip, None], track_of=TRACK_OF, faders=[0.9, 0.7], buses=[mc.comb],
                    track_sends=[[0.5, 0.25]], stems=stems, **kw)
    finally:
        d.configure(48000)


def stacked(got):
    return np.stack([np.stack(got[name]) for name in got.names])


@functools.lru_cache(maxsize=None)
def reference(stems=True):
    """the call with true_peak=True, once: its result and the f32 signals it delivers [S + 1, 2, NT]"""
    got = piece(true_peak=True, stems=stems)
    stack = stacked(got) if stems else np.stack(got.mix)[None]
    stack.setflags(write=False)
    return got, stack


def meters_dict(meters):
    return dict(rms=[meters.rms[k] for k in meters.names], momentary=[meters.momentary[k] for k in meters.names], lufs=[meters.lufs[k] for k in meters.names])


def one_step(a, b):
    return abs(float(a) - float(b)) <= float(np.spacing(np.float32(b)))


@pytest.mark.parametrize("depth", [16, 24])
def test_a_delivery_where_the_limiter_engages(depth, capsys):
    """the mix reads about -4.5 LUFS with a largest true peak of about 1.3: at a target of 0 LUFS under -1 dBTP the ceiling lies at about
    0.53 of the unlimited signals, so the limiter engages"""
    ref, stack = reference()
    taps = library_taps(RATE)
    got = piece(d.render_piece_pcm, depth, 0, loudness=0, true_peak_max=-1.0, limiter=True)
    lim = got.limiter
    assert isinstance(got, render.Stems) and isinstance(lim, render.Limiter) and got.names == ref.names
    assert lim.engaged is True and lim.window == WINDOW
    # what the limiter saw: the unlimited call's own loudness and largest true peak, bit for bit
    tp_in = np.stack([ref.meters.true_peak[k] for k in ref.names])
    assert bits64(lim.lufs_in) == bits64(ref.meters.lufs["mix"]) and lim.true_peak_in == tp_in.max() == mix.true_peak(stack, RATE, taps).max()
    want_T = mix.limiter_threshold(lim.lufs_in, 0.0, -1.0)
    assert abs(lim.threshold - want_T) <= np.spacing(want_T) and lim.true_peak_in > lim.threshold, (lim.threshold, want_T)
    # the limited signals, by the model at that threshold
    limited, g, reduction = mix.limit(stack, RATE, lim.threshold, WINDOW, taps)
    assert lim.reduction == reduction < 1.0
    tp = np.stack([got.meters.true_peak[k] for k in got.names])
    assert np.array_equal(bits64(tp), bits64(mix.true_peak(limited, RATE, taps))), "the true peaks are the limited signals'"
    mtc.held("limited", meters_dict(got.meters), mix.meters(limited, RATE), limited, RATE)
    lufs = got.meters.lufs["mix"]
    gain, level = mix.loudness_gain(lufs, tp, 0.0, -1.0)
    assert isinstance(got.level, np.float32) and one_step(got.level, level) and got.gain == 1.0 / float(np.float64(got.level))
    frames, peaks = wav.encode_at_level(limited, depth, got.level)
    for k, name in enumerate(got.names):
        assert got[name].data.tobytes() == frames[k].tobytes(), name
        assert np.float32(got[name].peak).view(np.uint32) == peaks[k].view(np.uint32) == np.float32(got.peaks[name]).view(np.uint32), "the peak is the limited signal's"
    # the whole chain by the model alone, from the f32 signals: the same decisions, and the figures to what the meters may differ by
    model = mix.deliver_limited(stack, RATE, 0.0, -1.0, WINDOW, taps)
    assert model["limiter"]["engaged"] and abs(model["limiter"]["threshold"] / lim.threshold - 1) < 1e-9 and abs(model["limiter"]["reduction"] / lim.reduction - 1) < 1e-9
    assert abs(model["gain"] / got.gain - 1) < 1e-6
    # what it is for: the delivery is louder than the one the ceiling alone gives, and still under the ceiling
    plain = piece(d.render_piece_pcm, depth, 0, loudness=0, true_peak_max=-1.0)
    ceiling = 10 ** (-1 / 20)
    with capsys.disabled():
        print("\nlimiter at %d bits: T %.6f, reduction %.6f, residual true peak %.6f x T; gain %.6f (without the limiter %.6f); delivered %.3f LUFS (without %.3f)"
              % (depth, lim.threshold, lim.reduction, tp.max() / lim.threshold, got.gain, plain.gain, lufs + 20 * math.log10(got.gain), plain.meters.lufs["mix"] + 20 * math.log10(plain.gain)))
    assert got.gain > plain.gain and tp.max() * got.gain <= ceiling * (1 + 2.0 ** -23) and tp.max() <= 1.01 * lim.threshold
    assert 0.0 > lufs + 20 * math.log10(got.gain) > plain.meters.lufs["mix"] + 20 * math.log10(plain.gain), "nearer the target, by what limiting did not take from the mix"
    # the stems still add up: the limited stems' f32 chain against the limited mix, to the bound derived in tests/test_limiter_host.py
    assert np.array_equal(bits32(mix.stems_sum(stack)), bits32(stack[-1])), "unlimited, the stems add up bit for bit"
    A = np.abs(limited[:-1].astype(np.float64)).sum(axis=0)  # (the magnitudes of the LIMITED stems)
    assert (np.abs(mix.stems_sum(limited).astype(np.float64) - limited[-1]) <= 2 * (len(stack) - 1) * 2.0 ** -24 * A).all()
    files = piece(d.render_piece_wav, depth, 0, loudness=0, true_peak_max=-1.0, limiter=True)
    assert files.level == got.level and files.gain == got.gain and files.mix == wav.encode_wav(got.mix.data, RATE, depth) and files.limiter.reduction == lim.reduction


def test_a_delivery_where_the_limiter_does_not_engage_is_the_one_without_it():
    with_limiter = piece(d.render_piece_pcm, 16, 0, loudness=-23, limiter=True, limiter_window=0.01)
    plain = piece(d.render_piece_pcm, 16, 0, loudness=-23)
    lim = with_limiter.limiter
    assert lim.engaged is False and lim.reduction == 1.0 and lim.window == 80 and not hasattr(plain, "limiter")
    assert lim.threshold > lim.true_peak_in > 1.0 and bits64(lim.lufs_in) == bits64(plain.meters.lufs["mix"])
    assert abs(lim.threshold - mix.limiter_threshold(lim.lufs_in, -23.0, -1.0)) <= np.spacing(lim.threshold)
    assert with_limiter.gain == plain.gain and with_limiter.level == plain.level and with_limiter.names == plain.names
    for name in plain.names:
        assert with_limiter[name].data.tobytes() == plain[name].data.tobytes() and with_limiter[name].peak == plain[name].peak
        assert np.array_equal(bits64(with_limiter.meters.true_peak[name]), bits64(plain.meters.true_peak[name])) and bits64(with_limiter.meters.lufs[name]) == bits64(plain.meters.lufs[name])
        assert np.array_equal(bits64(with_limiter.meters.rms[name]), bits64(plain.meters.rms[name])) and np.array_equal(bits64(with_limiter.meters.momentary[name]), bits64(plain.meters.momentary[name]))
    # a silent piece: the gain is unity, so the limiter is not engaged whatever the threshold says
    silent = piece(d.render_piece_pcm, 16, 0, gains=[0.0] * N, loudness=-16, limiter=True)
    assert silent.limiter.engaged is False and silent.gain == 1.0 and silent.limiter.lufs_in == -math.inf and silent.limiter.true_peak_in == 0.0


def test_without_stems_the_metered_form_and_the_score_call():
    ref, signal = reference(stems=False)
    taps = library_taps(RATE)
    lone = piece(d.render_piece_pcm, 24, 0, stems=False, loudness=-2, true_peak_max=-2, limiter=True)
    assert isinstance(lone, render.Metered) and lone.meters.names == ["mix"] and lone.limiter.engaged
    limited, _, reduction = mix.limit(signal, RATE, lone.limiter.threshold, WINDOW, taps)
    assert lone.limiter.reduction == reduction and np.array_equal(bits64(lone.meters.true_peak["mix"]), bits64(mix.true_peak(limited, RATE, taps)[0]))
    assert lone.mix.data.tobytes() == wav.encode_at_level(limited, 24, lone.level)[0][0].tobytes() and lone.mix.peak == wav.peak(limited)
    # render_score_pcm takes the same options: three isomorphic voices, no stems
    d.configure(RATE)
    try:
        voices = [d.Multiply(d.Osc(200 + 50 * k), 0.8) for k in range(3)]
        base = d.render_score(voices, [0, 800, 1600], 0.5, 1.0, true_peak=True)
        got = d.render_score_pcm(voices, [0, 800, 1600], 0.5, 1.0, 16, 0, loudness=0, limiter=True, limiter_window=0.002)
    finally:
        d.configure(48000)
    x = np.stack(base.mix)[None]
    assert got.limiter.engaged and got.limiter.window == 16
    limited, _, reduction = mix.limit(x, RATE, got.limiter.threshold, 16, taps)
    assert got.limiter.reduction == reduction and got.mix.data.tobytes() == wav.encode_at_level(limited, 16, got.level)[0][0].tobytes()


def test_the_refusals_of_the_piece_entry(monkeypatch):
    real = runtime.ScoreLimiter
    for window in (0, 4097):
        monkeypatch.setattr(runtime, "ScoreLimiter", lambda w, *where, window=window: real(window, *where))
        with pytest.raises(runtime.DuspHipError) as e:
            piece(d.render_piece_pcm, 16, 0, loudness=-16, limiter=True)
        assert "dusp_render_host_score_piece_limiter" in str(e.value) and "window is 1 .. 4096 samples, not %d" % window in str(e.value), str(e.value)
    monkeypatch.undo()
    # a limiter beside a loudness record that does not deliver
    real_loud = runtime.ScoreLoudness
    monkeypatch.setattr(runtime, "ScoreLoudness", lambda deliver, *rest: real_loud(0, *rest))
    with pytest.raises(runtime.DuspHipError, match="a limiter needs a loudness record with deliver = 1"):
        piece(d.render_piece_pcm, 16, 0, loudness=-16, limiter=True)
    monkeypatch.undo()
    # a refusal of the loudness record still comes first
    monkeypatch.setattr(runtime, "ScoreLimiter", lambda w, *where: real(0, *where))
    monkeypatch.setattr(runtime, "ScoreLoudness", lambda deliver, target, *rest: real_loud(deliver, math.nan, *rest))
    with pytest.raises(runtime.DuspHipError, match="loudness target must be a finite number"):
        piece(d.render_piece_pcm, 16, 0, loudness=-16, limiter=True)
    monkeypatch.undo()
    again = piece(d.render_piece_pcm, 16, 0, loudness=0, limiter=True)
    assert again.limiter.engaged, "a refused call leaves the next one whole"
