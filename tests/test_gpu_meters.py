"""Meters on the device (dusp_meter_device, dusp_meter_host, dusp_render_host_score_piece_meters).  The expected value
is the contract, mix.meters, over the f32 signals the call delivered; every figure is held to a bound worked out from the
coefficients and the number format (meter_cases.held): rms^2 within n 2^-52 of math.fsum, every block energy within
2 sqrt(C e) delta + C delta^2, the loudness within 10 log10(1 + rho) + 1e-12.  The delivered signals are bit for bit the call's without
meters.  Each test prints the largest observed ratio of an energy's difference to its bound; tests/test_meters_host.py anchors the
contract.

Measured on an MI355X: every case below passed; the largest observed ratio was 1.2e-4 (profiles/score_meters.txt lists one a test)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import meter_cases as mtc
import score_voices as sv
import send_cases as sc
import track_cases as tc
from dusp_amd import mix, render, runtime
from pan_cases import pans_for
from test_piece_host import NV_SAW, bits, interleaved_voice

pytestmark = pytest.mark.gpu

RATE = sv.SAMPLE_RATE
N = 13
NT = 5 * 4800 + 17  # a timeline of two blocks and a last short hop at 48 kHz; the voices end long before it does
DUR = (NT + 0.5) / RATE
SENTINEL = -77.25
GUARD = 64


def voices(n=N):
    return [interleaved_voice(k) for k in range(n)]


def durations(n=N):
    return [((sv.NV if k % 2 == 0 else NV_SAW) + 0.5) / RATE for k in range(n)]


# ---- dusp_meter_device alone ------------------------------------------------------------------------------------------------------------

def fenced(torch, n, skip, dtype):
    """n elements behind GUARD + skip sentinels and in front of GUARD more -> (the tensor, the address of the n elements, their slice)"""
    t = torch.full((GUARD + skip + n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    return t, t.data_ptr() + t.element_size() * (GUARD + skip), slice(GUARD + skip, GUARD + skip + n)


def untouched(t, inner):
    a = t.cpu().numpy()
    return (a[:inner.start] == SENTINEL).all() and (a[inner.stop:] == SENTINEL).all()


@functools.lru_cache(maxsize=None)
def device_case(kind, shape, n):
    x = {"noise": mtc.shaped_noise, "dc": mtc.dc_noise, "inf": lambda n, shape: mtc.planted_inf(n, shape)[0]}[kind](n, shape)
    want = mix.meters(x, 8000)
    x.setflags(write=False)
    return x, want


def from_sums(sumsq, hops, n, rate):
    """what the library's host part makes of the sums, by the contract's formulas: dict(rms, momentary, lufs)"""
    hop = mix.meter_hop(rate)
    n_blocks = mix.meter_blocks(n, rate)
    with np.errstate(all="ignore"):
        e = np.array([[(((h[j] + h[j + 1]) + h[j + 2]) + h[j + 3]) / (4 * hop) for j in range(n_blocks)] for h in hops]).reshape(len(hops), n_blocks)
        got = [mix.loudness(row) for row in e]
        return dict(rms=np.sqrt(sumsq / n), momentary=np.array([m for m, _ in got]).reshape(len(hops), n_blocks), lufs=np.array([l for _, l in got]))


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (12, 8)], ids=["1x1", "3x2", "12x8"])
@pytest.mark.parametrize("kind", ["noise", "dc", "inf"])
def test_the_meter_kernels_alone(kind, shape, capsys):
    """n below, at and above a hop and a block (8 kHz: hop 800, block 3200, segments of 400), buffers on and off 16-byte boundaries,
    fences around both outputs; two runs give the same bits"""
    import torch
    ctx = runtime.Context(-1, RATE)
    stream = torch.cuda.current_stream().cuda_stream
    S, C = shape
    worst = 0.0
    try:
        for n in (1, 799, 800, 3200, 3201, 3 * 3200 + 17):
            x, want = device_case(kind, shape, n)
            n_hops = -(-n // 800)
            seen = []
            for skip in (0, 1):  # (floats in front of the signals; doubles in front of the sums)
                d_x = torch.from_numpy(np.concatenate([np.zeros(skip, np.float32), x.ravel()])).cuda()
                (t_sq, p_sq, in_sq), (t_hops, p_hops, in_hops) = fenced(torch, S * C, skip, torch.float64), fenced(torch, S * n_hops, 1 - skip, torch.float64)
                assert (d_x.data_ptr() + 4 * skip) % 16 == (4 * skip) % 16
                ctx.meter_device(d_x.data_ptr() + 4 * skip, S, C, n, 8000, p_sq, p_hops, stream)
                torch.cuda.synchronize()
                assert untouched(t_sq, in_sq) and untouched(t_hops, in_hops), "a meter kernel wrote outside its output"
                sumsq, hops = t_sq.cpu().numpy()[in_sq].reshape(S, C), t_hops.cpu().numpy()[in_hops].reshape(S, n_hops)
                seen.append((sumsq, hops))
                worst = max(worst, mtc.held("%s %dx%d n %d" % (kind, S, C, n), from_sums(sumsq, hops, n, 8000), want, x, 8000))
                # below a block there is no block: the hop sums themselves, as energies of their hops
                z = mix.k_weighted(x.reshape(S * C, n), 8000).reshape(S, C, n) if n < 3200 else None
                for h in range(n_hops if z is not None else 0):
                    with np.errstate(all="ignore"):
                        w = z[:, :, h * 800:(h + 1) * 800]
                        e = (w * w).sum(axis=2).sum(axis=1) / w.shape[2]
                        fine = np.isfinite(e)
                        assert np.array_equal(np.isfinite(hops[:, h]), fine)
                        bound = mtc.energy_bound(e, C, mtc.sample_bound(8000, mtc.finite_peak(x))) + 1e-13 * e
                        assert np.all(np.abs(hops[fine, h] / w.shape[2] - e[fine]) <= bound[fine]), (kind, n, h)
            assert np.array_equal(bits64(seen[0][0]), bits64(seen[1][0])) and np.array_equal(bits64(seen[0][1]), bits64(seen[1][1])), "two runs, two results"
        k, _, _ = ctx.score_last_ms()
        passes = ctx.meter_last_ms()
        assert k > 0 and len(passes) == 4 and all(p >= 0 for p in passes)
    finally:
        ctx.close()
    with capsys.disabled():
        print("\nmeter kernels alone, %s %dx%d: largest |energy difference| / bound %.3g" % (kind, S, C, worst))


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_both_gates_on_the_device_and_render_meter_on_a_host_array(capsys):
    x = mtc.gated_noise()
    want = mix.meters(x, 8000)
    got = render.meter(x, 8000)
    assert got.names == ["0"] and got.momentary["0"].shape == (37,) and (got.hop, got.block) == (800, 3200)
    raw = dict(rms=[got.rms["0"]], momentary=[got.momentary["0"]], lufs=[got.lufs["0"]])
    worst = mtc.held("gated noise", raw, want, x, 8000)
    assert abs(got.lufs["0"] + 18.41) <= 0.01
    m = got.momentary["0"]
    assert np.array_equal(m > -70, want["momentary"][0] > -70), "the same blocks above the gate"
    # [channels, samples] is one signal; several signals and channels; an Inf
    ctx = runtime.Context(-1, RATE)
    try:
        one = ctx.meter(x[0], 8000)
        assert one["lufs"][0] == got.lufs["0"] and np.array_equal(one["momentary"][0], m)
        y, _ = mtc.planted_inf(3 * 3200 + 17, (3, 2))
        worst = max(worst, mtc.held("host array with an Inf", ctx.meter(y, 8000), mix.meters(y, 8000), y, 8000))
        z = mtc.dc_noise(44100 + 11, (2, 2))
        worst = max(worst, mtc.held("host array at 44.1 kHz", ctx.meter(z, 44100), mix.meters(z, 44100), z, 44100))
        with pytest.raises(ValueError) as e:
            ctx.meter(x, 7999)
        assert str(e.value) == mix.METER_RATE_LOW % 7999
    finally:
        ctx.close()
    with capsys.disabled():
        print("\nrender.meter: largest |energy difference| / bound %.3g" % worst)


# ---- pieces ------------------------------------------------------------------------------------------------------------------------------

def stacked(got):
    return np.stack([np.stack(got[name]) for name in got.names])


def as_raw(meters):
    return dict(rms=[meters.rms[k] for k in meters.names], momentary=[meters.momentary[k] for k in meters.names], lufs=[meters.lufs[k] for k in meters.names])


def same_meters(a, b):
    return a.names == b.names and all(np.array_equal(bits64(a.rms[k]), bits64(b.rms[k])) and np.array_equal(bits64(a.momentary[k]), bits64(b.momentary[k])) and
                                      bits64(a.lufs[k]) == bits64(b.lufs[k]) for k in a.names)


def tracks_piece(call=d.render_piece, *more, **kw):
    """track_cases' piece: a clip track, an echo track, a fader group and direct voices, two buses fed by the tracks"""
    onsets, _, gains = sv.layout(N)
    d.configure(RATE)
    return call(voices(), onsets, durations(), DUR, *more, lengths=None, gains=gains, tracks=[mc.clip, mc.echo, None], track_of=tc.track_of(N, 3), faders=tc.faders(3),
                buses=[mc.echo, mc.comb], track_sends=tc.levels(2, 3), **kw)


def test_a_piece_with_stems_and_meters(capsys):
    plain = tracks_piece(stems=True)
    got = tracks_piece(stems=True, meters=True)
    assert isinstance(got, render.Stems) and got.names == plain.names == ["direct", "track0", "track1", "track2", "bus0", "bus1", "mix"] and not hasattr(plain, "meters")
    stack = stacked(got)
    assert np.array_equal(bits(stack), bits(stacked(plain))), "the signals are the call's without meters"
    assert all(np.float32(got.peaks[k]).view(np.uint32) == np.float32(plain.peaks[k]).view(np.uint32) for k in got.names)
    m = got.meters
    assert m.names == got.names and (m.hop, m.block) == (4800, 19200) and all(m.momentary[k].shape == (2,) and m.rms[k].shape == (1,) for k in m.names)
    worst = mtc.held("tracks, buses, stems", as_raw(m), mix.meters(stack, RATE), stack, RATE)
    assert all(math.isfinite(m.lufs[k]) for k in ("direct", "track0", "mix")), m.lufs
    # the same meters with s16 and s24 frames in the three normalise modes: they are taken in front of the PCM gain
    for depth in (16, 24):
        for normalise in (0, 1, 2):
            pcm = tracks_piece(d.render_piece_pcm, depth, normalise, stems=True, meters=True)
            assert same_meters(pcm.meters, m), (depth, normalise)
            base = tracks_piece(d.render_piece_pcm, depth, normalise, stems=True)
            assert all(np.array_equal(pcm[k].data, base[k].data) for k in pcm.names) and pcm.gain == base.gain
    files = tracks_piece(d.render_piece_wav, 16, 1, stems=True, meters=True)
    assert same_meters(files.meters, m) and files.mix == tracks_piece(d.render_piece_wav, 16, 1, stems=True).mix
    # a call without meters afterwards is what it was
    after = tracks_piece(stems=True)
    assert not hasattr(after, "meters") and np.array_equal(bits(stacked(after)), bits(stack))
    with capsys.disabled():
        print("\npiece with stems and meters: largest |energy difference| / bound %.3g" % worst)


@pytest.mark.parametrize("how", ["plain", "master", "sends", "tracks", "stereo"])
def test_meters_without_stems_on_every_delivery_path(how, capsys):
    onsets, _, gains = sv.layout(N)
    d.configure(RATE)
    kw = {"plain": {}, "master": dict(master=mc.allpass), "sends": dict(buses=[mc.echo, mc.comb], sends=sc.levels(N, 2)),
          "tracks": dict(tracks=[mc.clip, None], track_of=tc.track_of(N, 2), faders=tc.faders(2), master=mc.echo),
          "stereo": dict(pans=pans_for(N))}[how]
    make = (lambda: [sv.voice(k) for k in range(N)]) if how == "stereo" else voices
    dur = (sv.NV + 0.5) / RATE if how == "stereo" else durations()
    plain = d.render_piece(make(), onsets, dur, DUR, None, gains, **kw)
    got = d.render_piece(make(), onsets, dur, DUR, None, gains, meters=True, **kw)
    assert isinstance(got, render.Metered) and got.meters.names == ["mix"] and got.mix.sampleRate == RATE
    signals = np.stack(got.mix)[None]
    assert np.array_equal(bits(signals[0]), bits(np.stack(plain))), "the mix is the call's without meters"
    assert signals.shape == (1, 2 if how == "stereo" else 1, NT) and got.meters.rms["mix"].shape == (signals.shape[1],)
    worst = mtc.held(how, as_raw(got.meters), mix.meters(signals, RATE), signals, RATE)
    pcm = d.render_piece_pcm(make(), onsets, dur, DUR, 24, 2, None, gains, meters=True, **kw)
    assert same_meters(pcm.meters, got.meters) and np.array_equal(pcm.mix.data, d.render_piece_pcm(make(), onsets, dur, DUR, 24, 2, None, gains, **kw).data)
    with capsys.disabled():
        print("\nmeters without stems, %s: largest |energy difference| / bound %.3g" % (how, worst))


def test_a_score_is_the_piece_of_its_one_part():
    onsets, _, gains = sv.layout(N)
    d.configure(RATE)
    mono = lambda: [sv.voice(k) for k in range(N)]
    kw = dict(buses=[mc.echo], sends=sc.levels(N, 1), master=mc.allpass, stems=True, meters=True)
    score = d.render_score(mono(), onsets, (sv.NV + 0.5) / RATE, DUR, None, gains, **kw)
    piece = d.render_piece(mono(), onsets, (sv.NV + 0.5) / RATE, DUR, None, gains, **kw)
    assert score.names == piece.names == ["direct", "bus0", "mix"] and np.array_equal(bits(stacked(score)), bits(stacked(piece))) and same_meters(score.meters, piece.meters)
    lone = d.render_score(mono(), onsets, (sv.NV + 0.5) / RATE, DUR, None, gains, meters=True)
    assert isinstance(lone, render.Metered) and same_meters(lone.meters, d.render_piece(mono(), onsets, (sv.NV + 0.5) / RATE, DUR, None, gains, meters=True).meters)


# ---- the refusals of the C entries, through ctypes ----------------------------------------------------------------------------------

def test_every_refusal_of_the_c_entries(monkeypatch):
    import torch
    ctx = runtime.Context(-1, RATE)
    L = ctx._L
    x = mtc.shaped_noise(4000, (2, 1))
    d_x, d_sq, d_hops = torch.from_numpy(x.ravel()).cuda(), torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(10, dtype=torch.float64, device="cuda")
    rms, lufs = np.zeros(2), np.zeros(2)

    def refused(rc, *words):
        message = L.dusp_last_error(ctx._h).decode()
        assert rc != 0 and all(w in message for w in words), (rc, message)

    try:
        refused(L.dusp_meter_device(ctx._h, d_x.data_ptr(), 2, 1, 4000, 7999, d_sq.data_ptr(), d_hops.data_ptr(), None), "dusp_meter_device", "at least 8000 Hz, not 7999")
        refused(L.dusp_meter_device(ctx._h, None, 2, 1, 4000, 8000, d_sq.data_ptr(), d_hops.data_ptr(), None), "dusp_meter_device: NULL buffer")
        refused(L.dusp_meter_device(ctx._h, d_x.data_ptr(), 2, 1, 4000, 8000, None, d_hops.data_ptr(), None), "NULL buffer")
        refused(L.dusp_meter_device(ctx._h, d_x.data_ptr(), 2, 0, 4000, 8000, d_sq.data_ptr(), d_hops.data_ptr(), None), "1..64 channels")
        refused(L.dusp_meter_device(ctx._h, d_x.data_ptr(), 2, 1, 0, 8000, d_sq.data_ptr(), d_hops.data_ptr(), None), "1..2^31 samples")
        refused(L.dusp_meter_device(ctx._h, d_x.data_ptr() + 2, 2, 1, 3999, 8000, d_sq.data_ptr(), d_hops.data_ptr(), None), "4-byte aligned")
        refused(L.dusp_meter_device(ctx._h, d_x.data_ptr(), 2, 1, 4000, 8000, d_sq.data_ptr() + 4, d_hops.data_ptr(), None), "8-byte aligned")
        refused(L.dusp_meter_host(ctx._h, x.ctypes.data, 2, 1, 4000, 7999, rms.ctypes.data, lufs.ctypes.data, None), "dusp_meter_host", "at least 8000 Hz, not 7999")
        refused(L.dusp_meter_host(ctx._h, x.ctypes.data, 2, 1, 4000, 8000, None, lufs.ctypes.data, None), "dusp_meter_host: NULL buffer")
        refused(L.dusp_meter_host(ctx._h, x.ctypes.data, 2, 1, 4000, 8000, rms.ctypes.data, None, None), "dusp_meter_host: NULL buffer")
        refused(L.dusp_meter_host(ctx._h, None, 2, 1, 4000, 8000, rms.ctypes.data, lufs.ctypes.data, None), "dusp_meter_host: NULL buffer")
        assert L.dusp_meter_host(ctx._h, x.ctypes.data, 2, 1, 4000, 8000, rms.ctypes.data, lufs.ctypes.data, None) == 0 and rms[0] > 0  # (h_momentary may be NULL)
        ms = (ctypes.c_float * 4)()
        refused(L.dusp_meter_last_ms(ctx._h, ctypes.addressof(ms)), "no dusp_meter_device call")
    finally:
        ctx.close()
    # the piece's entry: what the binding fills in rightly, bent one field at a time
    real = runtime.ScoreMeters

    def bent(**fields):
        def make(n_signals, n_blocks, h_rms, h_lufs, h_momentary):
            given = dict(n_signals=n_signals, n_blocks=n_blocks, h_rms=h_rms, h_lufs=h_lufs, h_momentary=h_momentary)
            given.update({k: (v(given[k]) if callable(v) else v) for k, v in fields.items()})
            return real(given["n_signals"], given["n_blocks"], given["h_rms"], given["h_lufs"], given["h_momentary"])
        return make

    for fields, stems, words in ((dict(n_signals=lambda v: v + 1), True, ("the meters' n_signals is 8, the call delivers 7",)),
                                 (dict(n_signals=7), False, ("the meters' n_signals is 7, the call delivers 1",)),
                                 (dict(n_blocks=lambda v: v + 3), True, ("the meters' n_blocks is 5", "has 2 blocks", "%d samples at 48000 Hz" % NT)),
                                 (dict(h_rms=None), True, ("h_rms is NULL",)),
                                 (dict(h_lufs=None), False, ("h_lufs is NULL",))):
        monkeypatch.setattr(runtime, "ScoreMeters", bent(**fields))
        with pytest.raises(runtime.DuspHipError) as e:
            tracks_piece(stems=stems, meters=True)
        assert "dusp_render_host_score_piece_meters" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    monkeypatch.setattr(runtime, "ScoreMeters", bent(h_momentary=None))  # (NULL allowed)
    got = tracks_piece(stems=True, meters=True)
    assert math.isfinite(got.meters.lufs["mix"]) and not got.meters.momentary["mix"].any()
    monkeypatch.setattr(runtime, "ScoreMeters", real)
    # a piece at a sample rate below 8000: the binding refuses it in the library's words; with the binding's own check out of the way the
    # library does, before anything renders
    try:
        d.configure(4000)
        low = lambda: d.render_piece([sv.voice(k) for k in range(3)], [0, 1, 2], 0.01, 0.05, meters=True)
        with pytest.raises(ValueError) as e:
            low()
        assert str(e.value) == mix.METER_RATE_LOW % 4000
        monkeypatch.setattr(runtime, "METER_RATE_MIN", 0)
        monkeypatch.setattr(mix, "METER_RATE_MIN", 0)
        with pytest.raises(runtime.DuspHipError) as e:
            low()
        assert "dusp_render_host_score_piece_meters: meters need a sample rate of at least 8000 Hz, not 4000" in str(e.value)
    finally:
        d.configure(RATE)
        monkeypatch.undo()
    assert same_meters(tracks_piece(stems=True, meters=True).meters, tracks_piece(stems=True, meters=True).meters)
