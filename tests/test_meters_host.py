"""Meters without a device: the contract mix.meters — the K-weighting's coefficients against the table of ITU-R
BS.1770-4, the block count, the standard's calibration sine, a case where both gates act, a planted Inf — the refusal string and the
routing of meters=, and the text of the meter kernels on the host under sanitizers (tests/native/meter_kernel_check.cpp)."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import meter_cases as mtc
import score_voices as sv
from dusp_amd import mix, render, runtime
from test_piece_host import ROOT, SANITIZE


def test_the_k_weighting_at_48_khz_is_the_standards_table():
    shelf, rlb = mix.k_weighting(48000)
    assert np.allclose(shelf, (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585), rtol=0, atol=1e-13)
    assert rlb[:3] == (1.0, -2.0, 1.0) and np.allclose(rlb[3:], (-1.99004745483398, 0.99007225036621), rtol=0, atol=1e-13)
    for rate in (8000, 11025, 44100, 192000):  # (stable at every rate the project renders at)
        for _, _, _, a1, a2 in mix.k_weighting(rate):
            assert abs(a2) < 1 and abs(a1) < 1 + a2
    for rate in (7999, 0, -1):
        with pytest.raises(ValueError) as e:
            mix.k_weighting(rate)
        assert str(e.value) == mix.METER_RATE_LOW % rate


def test_the_block_count():
    L = runtime.load()
    for rate, hop in ((8000, 800), (11025, 1103), (44100, 4410), (48000, 4800), (192000, 19200)):
        assert mix.meter_hop(rate) == hop
        block = 4 * hop
        for n, want in ((0, 0), (1, 0), (block - 1, 0), (block, 1), (block + hop - 1, 1), (block + hop, 2), (10 * block + 3, 37)):
            assert mix.meter_blocks(n, rate) == want, (rate, n)
            assert L.dusp_meter_blocks(n, rate) == want, (rate, n)
    assert L.dusp_meter_blocks(100000, 7999) == 0


def test_the_calibration_sine_reads_minus_3_01_lufs():
    """a 997 Hz sine of amplitude 1, 3 s, mono, 48 kHz: the standard's calibration point"""
    t = np.arange(3 * 48000) / 48000.0
    got = mix.meters(np.sin(2 * np.pi * 997 * t).astype(np.float32)[None, None], 48000)
    assert got["hop"] == 4800 and got["block"] == 19200 and got["momentary"].shape == (1, 27)
    assert abs(got["lufs"][0] + 3.01) <= 0.01, got["lufs"]
    assert abs(got["rms"][0, 0] - math.sqrt(0.5)) < 1e-6
    assert np.all(np.abs(got["momentary"][0] + 3.01) <= 0.01)


def test_both_gates_act_and_no_block_lies_near_one():
    x = mtc.gated_noise()
    assert x.shape == (1, 1, 32123)
    got = mix.meters(x, 8000)
    m, e = got["momentary"][0], got["energies"][0]
    assert m.shape == (37,) and abs(got["lufs"][0] + 18.41) <= 0.01, got["lufs"]
    kept = m > -70
    gamma = -0.691 + 10 * math.log10(e[kept].mean()) - 10
    both = kept & (m > gamma)
    assert 0 < (~kept).sum() and 0 < (kept & ~both).sum() and 0 < both.sum(), "both gates remove a block"
    assert abs(gamma + 28.4) < 0.3  # (about -28.4: ten below the loudness of the blocks above -70)
    # no block within 0.5 LU of either gate: a rounding cannot move one across
    assert np.all(np.abs(m + 70) > 0.5) and np.all(np.abs(m[kept] - gamma) > 0.5), (np.sort(np.abs(m + 70))[:2], np.sort(np.abs(m[kept] - gamma))[:2])
    assert got["lufs"][0] == -0.691 + 10 * math.log10(e[both].mean())
    # every channel has weight 1: the same signal on two channels is twice the energy
    two = mix.meters(np.repeat(x, 2, axis=1), 8000)
    assert np.allclose(two["energies"], 2 * got["energies"], rtol=1e-15) and np.array_equal(two["rms"][0], [got["rms"][0, 0]] * 2)
    # silence: no block above the gate; less than a block: no block at all
    assert mix.meters(np.zeros((1, 1, 4000), dtype=np.float32), 8000)["lufs"][0] == -math.inf
    short = mix.meters(x[:, :, :3199], 8000)
    assert short["momentary"].shape == (1, 0) and short["lufs"][0] == -math.inf and short["rms"][0, 0] > 0


def test_a_planted_inf_makes_every_block_from_it_on_not_finite():
    x, at = mtc.planted_inf(3 * 3200 + 17, (2, 2))
    got = mix.meters(x, 8000)
    first = max(0, (at - 3200) // 800 + 1)  # the first block that holds the sample
    e = got["energies"]
    assert np.all(np.isfinite(e[0])) and math.isfinite(got["lufs"][0])
    assert 0 < first < e.shape[1] and np.all(np.isfinite(e[1, :first])) and not np.any(np.isfinite(e[1, first:]))
    assert math.isnan(got["lufs"][1]) and not math.isfinite(got["rms"][1, 1]) and math.isfinite(got["rms"][1, 0])
    # the rows of many signals go through numpy a step, the rows of few through Python's doubles: the same operations
    many = np.random.default_rng(5).standard_normal((16, 700)).astype(np.float32)
    assert np.array_equal(mix.k_weighted(many, 8000)[:3], mix.k_weighted(many[:3], 8000))


# ---- the Python surface, without a device -----------------------------------------------------------------------------------------------

CALLS = (d.render_piece, d.render_score, d.render_piece_pcm, d.render_score_pcm, d.render_piece_wav, d.render_score_wav)


def voices(n=3):
    d.configure(sv.SAMPLE_RATE)
    return [sv.voice(k) for k in range(n)]


@pytest.mark.parametrize("call", CALLS, ids=lambda f: f.__name__)
def test_meters_that_is_no_bool_is_refused_by_string_next_to_stems(call):
    for value in (1, 0, None, "lufs", ["mix"], 2.0):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, meters=value, pans=[0])  # (the pans' shape would be refused next)
        assert str(e.value) == mix.METERS_NOT_BOOL
    with pytest.raises(ValueError) as e:
        call(voices(), [0, 1, 2], 0.01, 0.05, meters=1, stems=1)
    assert str(e.value) == mix.STEMS_NOT_BOOL  # (stems first)
    assert mix.check_meters(True) is True and mix.check_meters(np.bool_(False)) is False


def test_meters_travel_with_the_placement_to_the_piece():
    d.configure(sv.SAMPLE_RATE)
    assert render._placing(None, None, None, None, -3, None, False)["meters"] is False
    placing = render._placing(None, None, None, None, -3, None, False, None, [mc.echo], None, [mc.clip, None], [1, -1, 0], None, [[1, 0.5]], True, True)
    assert placing["meters"] is True and placing["stems"] is True
    *_, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, placing)
    assert place.meters is True and place.stems is True and "meters" not in place.keywords()
    *_, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, render._placing(None, None, None, None, -3, None, False, meters=True))
    assert place.meters is True and place.stems is False
    # a score with meters goes the piece's way, as one part
    with pytest.raises(d.DuspError, match="the voices of a score are isomorphic circuits"):
        d.render_score([sv.voice(0), mc.stereo_voice(1)], [0, 1], 0.01, 0, meters=True)
    # a timeline of no samples renders nothing: no energy and no block, by name
    with_tracks = dict(tracks=[mc.echo, None], track_of=[0, 1, -1], faders=[1, 0.5], buses=[mc.comb], track_sends=[[1, 0]])
    got = d.render_score(voices(), [0, 1, 2], 0.01, 0, stems=True, meters=True, **with_tracks)
    assert isinstance(got, render.Stems) and isinstance(got.meters, render.Meters) and got.meters.names == got.names == mix.stem_names(2, 1)
    assert all(got.meters.lufs[name] == -math.inf and got.meters.momentary[name].shape == (0,) and np.array_equal(got.meters.rms[name], [0.0]) for name in got.names)
    assert (got.meters.hop, got.meters.block) == (4800, 19200)
    one = d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 2, meters=True)
    assert isinstance(one, render.Metered) and one.meters.names == ["mix"] and one.mix.data.shape == (0, 1, 3) and one.meters.lufs["mix"] == -math.inf
    files = d.render_piece_wav(voices(), [0, 1, 2], 0.01, 0, 16, 0, stems=True, meters=True, **with_tracks)
    assert files.meters.names == got.names and files.mix[:4] == b"RIFF"
    assert d.render_score_wav(voices(), [0, 1, 2], 0.01, 0, 16, 0, meters=True).mix[:4] == b"RIFF"
    # without meters a call hands back what it did
    assert not hasattr(d.render_score(voices(), [0, 1, 2], 0.01, 0, stems=True, **with_tracks), "meters")
    assert len(d.render_piece(voices(), [0, 1, 2], 0.01, 0, meters=False)) == 0


# ---- the kernels' text, under sanitizers ------------------------------------------------------------------------------------------------

def test_meter_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/meter_engine.hip itself, compiled for the host — the lanes of a workgroup as threads, LDS as statics, __syncthreads
    a barrier (tests/native/hip_host_stub_lds) — every buffer a heap allocation of exactly its size, under AddressSanitizer and UBSan,
    against the one sequential loop (tests/native/meter_kernel_check.cpp lists what it covers).  A stand-alone program, run as a
    subprocess; nothing is loaded into Python under a sanitizer."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "meter_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub_lds"), "-x", "c++",
                           os.path.join(native, "meter_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 1500 and rep["groups"] > 700 and rep["worst"] <= 1.0, rep
