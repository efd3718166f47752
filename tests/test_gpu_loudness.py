"""Loudness delivery on the device (dusp_true_peak_device, dusp_true_peak_host, dusp_render_host_score_piece_loudness).
The true-peak kernel is held BIT FOR BIT to the contract, mix.true_peak fed the library's own taps: the kernel forms every product and
sum in the contract's order, unfused, and an unsigned maximum commutes, so there is nothing to bound.  A call with true_peak=True is the
call with meters=True bit for bit, plus the true peaks of the f32 signals it delivers; a call with loudness= delivers the bytes of
wav.encode_at_level over those signals at the level it returns, which is mix.loudness_gain's over the loudness and true peaks it
returns, to one f32 step (the library's pow and Python's may differ in the last place).

Measured on an MI355X: every case below passed.  The piece's mix reads -4.47 LUFS with a largest true peak of 1.296 (the clip track's
overshoot); loudness=-23 returned level 8.440889 = the contract's, gain 0.118470929; loudness=0 under -1 dBTP returned gain 0.687533394,
the largest true peak leaving at 0.891250918 against a ceiling of 0.891250938: 2.3e-8 below it (level is 1 / G rounded to the nearest
f32, here upwards; a level that rounds downwards would land as far above)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
from dusp_amd import descriptor, mix, render, runtime, wav

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA15EA15EA15EA1
GUARD = 16
RATES = {44100: (4, 13), 96000: (2, 25), 192000: (1, 1)}


def library_taps(rate):
    factor, h49 = ctypes.c_int(0), (ctypes.c_double * 49)()
    assert runtime.load().dusp_true_peak_taps(rate, ctypes.byref(factor), h49) == 0
    return factor.value, np.array(h49[:] if factor.value > 1 else h49[:1])


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def case(kind, shape, n, rate):
    """-> (signals float32 [S, C, n], the contract's true peaks as words uint64 [S, C])"""
    S, C = shape
    x = (0.2 * np.random.default_rng(n * 7 + S * 3 + C + len(kind)).standard_normal((S, C, n))).astype(np.float32)
    if kind == "last":
        x[:, :, -1] = 0.95  # (the peak lies in the tail, u >= n)
    elif kind == "first":
        x[:, :, 0] = -0.95
    elif kind in ("nan", "inf"):
        x[S - 1, 0, n // 2] = np.nan if kind == "nan" else -np.inf
    want = bits64(mix.true_peak(x, rate, taps=library_taps(rate)))
    x.setflags(write=False)
    return x, want


def device_words(torch, ctx, x, rate, skip):
    """dusp_true_peak_device over x placed `skip` floats behind a 16-byte boundary, its words between fences -> uint64 [S, C]"""
    S, C, n = x.shape
    d_x = torch.from_numpy(np.concatenate([np.zeros(skip, np.float32), x.ravel()])).cuda()
    d_w = torch.from_numpy(np.full(GUARD + S * C + GUARD, SENTINEL, dtype=np.uint64).view(np.int64)).cuda()
    ctx.true_peak_device(d_x.data_ptr() + 4 * skip, S, C, n, rate, d_w.data_ptr() + 8 * GUARD, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    w = d_w.cpu().numpy().view(np.uint64)
    assert (w[:GUARD] == SENTINEL).all() and (w[GUARD + S * C:] == SENTINEL).all(), "the true-peak kernel wrote outside its words"
    return w[GUARD:GUARD + S * C].reshape(S, C)


@pytest.mark.parametrize("rate", sorted(RATES))
def test_the_true_peak_kernel_is_the_contract_bit_for_bit(rate):
    """n = 1, below K - 1, around the tile W and where the halo and the tail cross a tile; rows on and off 16-byte boundaries; three
    signals of two channels; the peak in the tail and at the first sample; a NaN and an Inf make their own row NaN and no other; two
    runs give equal words; the host round trip gives the same doubles"""
    import torch
    F, K = RATES[rate]
    assert library_taps(rate)[0] == F
    ctx = runtime.Context(-1, 48000)
    try:
        W = ctx.true_peak_tile(1, 1, 1000, rate)
        assert W == 256  # (a short call: a position a lane)
        for n in sorted({1, 5, W - 1, W, W + 1, W + K - 2, W + K - 1}):
            shapes = [(1, 1), (3, 2)] + ([(1, 2)] if n % 2 else [])  # (odd n: the second row starts off a 16-byte boundary)
            for shape in shapes:
                for kind in ("noise", "last", "first", "nan", "inf"):
                    if (n == 1 and kind in ("last", "first")) or (shape == (1, 2) and kind in ("nan", "inf")):
                        continue
                    x, want = case(kind, shape, n, rate)
                    assert ctx.true_peak_tile(shape[0], shape[1], n, rate) == W
                    got = [device_words(torch, ctx, x, rate, skip) for skip in (0, 1)]
                    assert np.array_equal(got[0], got[1]), "two runs, two results"
                    assert np.array_equal(got[0], want), (rate, n, shape, kind, got[0], want)
                    if kind in ("nan", "inf"):
                        planted = np.zeros(shape, dtype=bool)
                        planted[-1, 0] = True
                        assert np.array_equal(np.isnan(got[0].view(np.float64)), planted), "that row only"
                    if kind == "last" and F > 1:
                        assert np.all(got[0].view(np.float64) >= np.float32(0.95))  # (phase 0 gives the last sample back at u = n - 1 + (K - 1) / 2)
        x, want = case("noise", (3, 2), W + K - 1, rate)
        assert np.array_equal(bits64(ctx.true_peak(x, rate)), want) and np.array_equal(bits64(render.true_peak(x[0], rate)), want[:1])
        k, _, _ = ctx.score_last_ms()
        assert k > 0
    finally:
        ctx.close()


def test_a_long_call_takes_more_positions_a_lane_and_gives_the_same_bits():
    """enough rows and samples that the grid rule gives a lane 2, 4 or 8 positions: whatever the tile, the contract's bits"""
    import torch
    ctx = runtime.Context(-1, 48000)
    try:
        seen = set()
        for shape, n in (((3, 2), 350001), ((3, 2), 90001), ((2, 2), 66001)):
            W = ctx.true_peak_tile(shape[0], shape[1], n, 44100)
            assert W in (256, 512, 1024, 2048)
            seen.add(W)
            x, want = case("last", shape, n, 44100)
            assert np.array_equal(device_words(torch, ctx, x, 44100, 1), want), (shape, n, W)
        assert len(seen) > 1 and max(seen) > 256, seen
    finally:
        ctx.close()


def test_every_refusal_of_the_true_peak_entries():
    import torch
    ctx = runtime.Context(-1, 48000)
    L = ctx._L
    x = np.zeros((2, 1, 400), dtype=np.float32)
    d_x, d_w = torch.from_numpy(x.ravel()).cuda(), torch.zeros(4, dtype=torch.int64, device="cuda")
    out = np.zeros(2)

    def refused(rc, *words):
        message = L.dusp_last_error(ctx._h).decode()
        assert rc != 0 and all(w in message for w in words), (rc, message)

    try:
        refused(L.dusp_true_peak_device(ctx._h, d_x.data_ptr(), 2, 1, 400, 0, d_w.data_ptr(), None), "dusp_true_peak_device", "needs a sample rate, not 0")
        refused(L.dusp_true_peak_device(ctx._h, None, 2, 1, 400, 8000, d_w.data_ptr(), None), "dusp_true_peak_device: NULL buffer")
        refused(L.dusp_true_peak_device(ctx._h, d_x.data_ptr(), 2, 1, 400, 8000, None, None), "NULL buffer")
        refused(L.dusp_true_peak_device(ctx._h, d_x.data_ptr(), 2, 0, 400, 8000, d_w.data_ptr(), None), "1..64 channels")
        refused(L.dusp_true_peak_device(ctx._h, d_x.data_ptr(), 2, 1, 0, 8000, d_w.data_ptr(), None), "1..2^31 samples")
        refused(L.dusp_true_peak_device(ctx._h, d_x.data_ptr() + 2, 2, 1, 399, 8000, d_w.data_ptr(), None), "4-byte aligned")
        refused(L.dusp_true_peak_device(ctx._h, d_x.data_ptr(), 2, 1, 400, 8000, d_w.data_ptr() + 4, None), "8-byte aligned")
        refused(L.dusp_true_peak_host(ctx._h, x.ctypes.data, 2, 1, 400, 0, out.ctypes.data), "dusp_true_peak_host", "not 0")
        refused(L.dusp_true_peak_host(ctx._h, None, 2, 1, 400, 8000, out.ctypes.data), "dusp_true_peak_host: NULL buffer")
        refused(L.dusp_true_peak_host(ctx._h, x.ctypes.data, 2, 1, 400, 8000, None), "dusp_true_peak_host: NULL buffer")
        assert L.dusp_true_peak_host(ctx._h, x.ctypes.data, 2, 1, 400, 100, out.ctypes.data) == 0 and out.tolist() == [0.0, 0.0]  # (no lower bound on the rate)
        assert L.dusp_true_peak_tile(ctx._h, 2, 1, 400, 0) == 0
    finally:
        ctx.close()


# ---- the call -----------------------------------------------------------------------------------------------------------------------------

RATE = 8000
NT = 8017  # about a second: two blocks and a last short hop at 8 kHz; odd, so that the second channel's rows start off a 16-byte boundary
N = 5
ONSETS = [0, 700, 1900, 2500, 3300]
PANS = [-0.6, 0.3, 0.0, 0.8, -0.2]
TRACK_OF = [0, 1, -1, 0, 1]


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


def same_but_true_peak(a, b):
    return a.names == b.names and (a.hop, a.block) == (b.hop, b.block) and all(
        np.array_equal(bits64(a.rms[k]), bits64(b.rms[k])) and np.array_equal(bits64(a.momentary[k]), bits64(b.momentary[k])) and bits64(a.lufs[k]) == bits64(b.lufs[k])
        for k in a.names)


@functools.lru_cache(maxsize=None)
def reference(scale=0.4):
    """the call with true_peak=True, once: its Stems, the f32 signals [S + 1, 2, NT] and all their true peaks by the contract"""
    got = piece(true_peak=True, scale=scale)
    stack = stacked(got)
    stack.setflags(write=False)
    return got, stack, mix.true_peak(stack, RATE, taps=library_taps(RATE))


def test_true_peak_beside_the_meters_of_a_piece_with_stems():
    got, stack, want = reference()
    assert got.names == ["direct", "track0", "track1", "bus0", "mix"] and stack.shape == (5, 2, NT)
    tp = np.stack([got.meters.true_peak[k] for k in got.names])
    assert np.array_equal(bits64(tp), bits64(want)), "the true peaks are the contract's over the delivered f32 signals"
    assert np.all(tp >= np.abs(stack).max(axis=2)) and np.all(tp > 0), "a true peak is no less than the sample peak"
    base = piece(meters=True)
    assert np.array_equal(stacked(base).view(np.uint32), stack.view(np.uint32)) and same_but_true_peak(base.meters, got.meters) and not hasattr(base.meters, "true_peak")
    assert all(np.float32(got.peaks[k]).view(np.uint32) == np.float32(base.peaks[k]).view(np.uint32) for k in got.names) and not hasattr(got, "level")
    # PCM with true peaks and no target: the frames, peaks and gain of the call with meters
    for depth, normalise in ((16, 2), (24, 1)):
        pcm, plain = piece(d.render_piece_pcm, depth, normalise, true_peak=True), piece(d.render_piece_pcm, depth, normalise, meters=True)
        assert all(np.array_equal(pcm[k].data, plain[k].data) and pcm[k].peak == plain[k].peak for k in pcm.names) and pcm.gain == plain.gain
        assert np.array_equal(bits64(np.stack([pcm.meters.true_peak[k] for k in pcm.names])), bits64(want)) and same_but_true_peak(pcm.meters, got.meters)


@pytest.mark.parametrize("depth", [16, 24])
def test_a_delivery_where_the_loudness_limits(depth, capsys):
    ref, stack, want_tp = reference()
    got = piece(d.render_piece_pcm, depth, 0, loudness=-23)
    assert isinstance(got, render.Stems) and got.names == ref.names and same_but_true_peak(got.meters, ref.meters)
    tp = np.stack([got.meters.true_peak[k] for k in got.names])
    assert np.array_equal(bits64(tp), bits64(want_tp))
    lufs = got.meters.lufs["mix"]
    gain, level = mix.loudness_gain(lufs, tp, -23.0, -1.0)
    with capsys.disabled():
        print("\nloudness -23 at %d bits: mix %.4f LUFS, largest true peak %.6f, level %r (the contract's %r), gain %.9f" % (depth, lufs, tp.max(), got.level, level, got.gain))
    assert math.isfinite(lufs) and 10 ** ((-23.0 - lufs) / 20) < 10 ** (-1 / 20) / tp.max(), "the loudness limits"
    assert isinstance(got.level, np.float32) and abs(float(got.level) - float(level)) <= float(np.spacing(level)), (got.level, level)
    assert got.gain == 1.0 / float(np.float64(got.level))
    assert abs(lufs + 20 * math.log10(got.gain) + 23.0) <= 1e-6
    frames, peaks = wav.encode_at_level(stack, depth, got.level)
    for k, name in enumerate(got.names):
        assert got[name].data.tobytes() == frames[k].tobytes(), name
        assert np.float32(got[name].peak).view(np.uint32) == peaks[k].view(np.uint32) == np.float32(ref.peaks[name]).view(np.uint32), "the peak stays the sample peak"
    assert frames.tobytes() != wav.encode_stems(stack, depth, 0)[0].tobytes()  # (a gain that is not 1 was applied)
    files = piece(d.render_piece_wav, depth, 0, loudness=-23)
    assert files.level == got.level and files.gain == got.gain and files.mix == wav.encode_wav(got.mix.data, RATE, depth)


def test_a_delivery_where_the_ceiling_limits(capsys):
    ref, stack, want_tp = reference()
    got = piece(d.render_piece_pcm, 16, 0, loudness=0, true_peak_max=-1.0)
    tp = np.stack([got.meters.true_peak[k] for k in got.names])
    ceiling = 10 ** (-1 / 20)
    gain, level = mix.loudness_gain(got.meters.lufs["mix"], tp, 0.0, -1.0)
    reached = tp.max() * got.gain
    with capsys.disabled():
        print("\nloudness 0 under -1 dBTP: largest true peak %.9f x gain %.9f = %.12f, the ceiling %.12f (ratio - 1 = %.3g)" % (tp.max(), got.gain, reached, ceiling, reached / ceiling - 1))
    assert 10 ** ((0.0 - got.meters.lufs["mix"]) / 20) > ceiling / tp.max(), "the ceiling limits"
    assert abs(float(got.level) - float(level)) <= float(np.spacing(level)) and got.gain == 1.0 / float(np.float64(got.level))
    assert ceiling * (1 - 2.0 ** -23) <= reached <= ceiling, "within one f32 step below the ceiling"
    frames, _ = wav.encode_at_level(stack, 16, got.level)
    assert all(got[name].data.tobytes() == frames[k].tobytes() for k, name in enumerate(got.names))
    assert max(int(np.abs(got[name].data.astype(np.int32)).max()) for name in got.names) < 32767, "no sample is clamped"
    assert np.abs(stack).max() * got.gain < 1.0


def test_without_stems_the_metered_form_and_a_silent_piece():
    lone = piece(d.render_piece_pcm, 24, 0, stems=False, loudness=-16, true_peak_max=-2)
    assert isinstance(lone, render.Metered) and lone.meters.names == ["mix"]
    planar = piece(stems=False, true_peak=True)
    signal = np.stack(planar.mix)[None]
    tp = mix.true_peak(signal, RATE, taps=library_taps(RATE))
    assert np.array_equal(bits64(lone.meters.true_peak["mix"]), bits64(tp[0])) and np.array_equal(bits64(planar.meters.true_peak["mix"]), bits64(tp[0]))
    _, level = mix.loudness_gain(lone.meters.lufs["mix"], tp, -16.0, -2.0)
    assert abs(float(lone.level) - float(level)) <= float(np.spacing(level)) and lone.gain == 1.0 / float(np.float64(lone.level)) and lone.gain != 1.0
    assert lone.mix.data.tobytes() == wav.encode_at_level(signal, 24, lone.level)[0][0].tobytes() and lone.mix.peak == wav.peak(signal)
    # a silent piece (every note times a gain of 0): no loudness to scale by, the gain is unity and the frames are the samples'
    silent = piece(d.render_piece_pcm, 16, 0, gains=[0.0] * N, loudness=-16)
    assert silent.gain == 1.0 and silent.level == np.float32(1.0) and silent.meters.lufs["mix"] == -math.inf
    assert all(np.array_equal(silent.meters.true_peak[k], [0.0, 0.0]) and not silent[k].data.any() and silent[k].data.shape == (NT, 2) for k in silent.names)


def test_the_refusals_of_the_piece_entry(monkeypatch):
    real = runtime.ScoreLoudness

    def bent(**fields):
        def make(deliver, target, ceiling, h_true_peak, h_gain, h_level):
            given = dict(deliver=deliver, target=target, ceiling=ceiling, h_true_peak=h_true_peak, h_gain=h_gain, h_level=h_level)
            given.update(fields)
            return real(given["deliver"], given["target"], given["ceiling"], given["h_true_peak"], given["h_gain"], given["h_level"])
        return make

    for fields, words in ((dict(h_true_peak=None), ("h_true_peak is NULL",)), (dict(target=math.nan), ("loudness target must be a finite number", "nan")),
                          (dict(target=math.inf), ("loudness target must be a finite number", "inf")), (dict(ceiling=0.5), ("ceiling must be a finite number of dBTP at most 0", "0.5")),
                          (dict(ceiling=math.nan), ("ceiling must be a finite number of dBTP at most 0", "nan"))):
        monkeypatch.setattr(runtime, "ScoreLoudness", bent(**fields))
        with pytest.raises(runtime.DuspHipError) as e:
            piece(d.render_piece_pcm, 16, 0, loudness=-16)
        assert "dusp_render_host_score_piece_loudness" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    monkeypatch.setattr(runtime, "ScoreLoudness", bent(deliver=1, target=-16.0))  # (deliver with format 0: the planar call)
    with pytest.raises(runtime.DuspHipError, match="needs a PCM format, not 0"):
        piece(true_peak=True)
    monkeypatch.setattr(runtime, "check_loudness", lambda loudness, ceiling, normalise, pcm: (loudness, ceiling))  # (deliver with normalise 2)
    monkeypatch.setattr(runtime, "ScoreLoudness", real)
    with pytest.raises(runtime.DuspHipError, match="does not go with normalise 2"):
        d.configure(RATE)
        ctx = render.context(RATE, -1)
        prog = ctx.build(descriptor.extract(d.Osc(200)).words)
        try:
            ctx.render_score_parts([(prog, 100, 1, None)], [0], [0], 4000, format="s16", normalise=2, loudness=-16.0)
        finally:
            prog.close()
            d.configure(48000)
    monkeypatch.undo()
    # an existing refusal still comes first: the meters' n_blocks bent together with a NULL h_true_peak
    monkeypatch.setattr(runtime, "ScoreLoudness", bent(h_true_peak=None))
    real_meters = runtime.ScoreMeters
    monkeypatch.setattr(runtime, "ScoreMeters", lambda n_signals, n_blocks, *arrays: real_meters(n_signals, n_blocks + 1, *arrays))
    with pytest.raises(runtime.DuspHipError, match="the meters' n_blocks is"):
        piece(true_peak=True)
    monkeypatch.undo()
    ref, _, want = reference()
    assert np.array_equal(bits64(np.stack([piece(true_peak=True).meters.true_peak[k] for k in ref.names])), bits64(want)), "a refused call leaves the next one whole"
