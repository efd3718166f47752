"""Sample rates other than 44.1 and 48 kHz, without a GPU.

The rate selects code paths: the oscillators' half-table image goes into LDS only at even rates and where it fits (99 KB at
48 kHz, 182 KB at 88.2 kHz, 198 KB at 96 kHz, 270 KB at 2^17 Hz: a workgroup has 160 KiB), the saw / square / triangle closed
forms hold only at some rates, and the wave engine and the circuit compiler refuse rates above 2^17.  The reference defines all
of its tables at every rate.  tests/golden/*_sr{8000,11025,22050,32000,96000,192000}* were written by the reference at those
rates (oracle/js/gen_golden.js --sampleRate=R); tests/test_gpu_sample_rates.py renders them on the device."""
import hashlib
import json
import os

import numpy as np
import pytest

import cases
import dusp_amd as d
from conftest import GOLDEN, Golden, golden_names
from dusp_amd import descriptor, runtime
from dusp_amd.wavetables import N_TABLES, TABLE_NAMES, make_table

GOLDEN_RATES = [8000, 11025, 22050, 32000, 96000, 192000]
RATE_GOLDEN = [name for sr in GOLDEN_RATES for name in golden_names(sr)]
# every rate a branch depends on: odd, 2 mod 4, ordinary, the image fits / does not fit LDS, exactly 2^17, above it
COMPILE_RATES = [8000, 11025, 22050, 32000, 44100, 48000, 88200, 96000, 131072, 192000]


def test_every_rate_has_the_same_cases():
    names = {sr: [n[: n.rindex("_sr")] for n in golden_names(sr)] for sr in GOLDEN_RATES}
    assert all(len(v) == 21 for v in names.values()) and len({tuple(sorted(v)) for v in names.values()}) == 1
    for n in RATE_GOLDEN:  # (each fixture no larger than the biggest at 48 kHz)
        for ext in (".json", ".desc.f64", ".pcm.f32"):
            assert os.path.getsize(os.path.join(GOLDEN, n + ext)) <= 192000, n + ext


@pytest.mark.parametrize("name", RATE_GOLDEN)
def test_oracle_matches_reference_at_other_rates(oracle, name):
    g = Golden(name)
    assert g.sample_rate == int(name[name.rindex("_sr") + 3:])
    pcm = oracle.render(g.desc, g.n_samples)
    assert pcm.shape == (g.n_channels, g.n_samples)
    assert g.windowed(pcm).tobytes() == g.pcm.tobytes()
    assert hashlib.sha256(pcm.tobytes()).hexdigest() == g.meta["sha256_full"]


def _reference_tables(sr):
    with open(os.path.join(GOLDEN, "wavetables_sr%d.json" % sr)) as f:
        meta = json.load(f)
    assert meta["sample_rate"] == sr
    return meta["tables"]


@pytest.mark.parametrize("sr", GOLDEN_RATES)
def test_oracle_and_host_tables_are_the_references(oracle, sr):
    """All nine tables at every rate, in the oracle and in what the Python host uploads — the reference defines each of them, the
    square and the triangle at odd rates and at rates of 2 mod 4 included (see test_tables_at_rates_not_divisible_by_four)."""
    meta = _reference_tables(sr)
    assert len(TABLE_NAMES) == N_TABLES == 9
    for tid, w in enumerate(TABLE_NAMES):
        mine, theirs = make_table(tid, sr), oracle.wavetable(tid, sr)
        assert mine.dtype == np.float32 and mine.size == theirs.size == meta[w]["length"] == sr + 1
        assert hashlib.sha256(theirs.tobytes()).hexdigest() == meta[w]["sha256"], w
        assert mine.tobytes() == theirs.tobytes(), w
        assert [float(x) for x in mine[:4]] == meta[w]["head"] and [float(x) for x in mine[-2:]] == meta[w]["tail"], w


@pytest.mark.parametrize("sr", [11025, 22050, 22051, 44099, 8002])
def test_tables_at_rates_not_divisible_by_four(oracle, sr):
    """The reference fills the square with fill(1, 0, sr / 2) — a typed array's fill truncates its bounds — and the triangle by
    quarters of sr / 4, where a store to a fractional index is dropped: the host serves exactly those tables, it does not refuse them."""
    sq = make_table(2, sr)
    assert np.all(sq[: sr // 2] == 1) and np.all(sq[sr // 2:] == -1)
    tri = make_table(3, sr).astype(np.float64)
    q = (sr + 3) // 4  # t = 0 .. ceil(sr / 4) - 1
    want = np.zeros(sr + 1)
    want[:q] = np.float32(np.arange(q) / sr * 4)
    if sr % 2 == 0:  # 2 (sr / 4) is whole: the third quarter, negated
        want[sr // 2: sr // 2 + q] = -want[:q]
    assert np.array_equal(tri, want) and np.array_equal(oracle.wavetable(3, sr), tri.astype(np.float32))
    assert np.signbit(make_table(3, sr)[sr // 2]) == (sr % 2 == 0)  # (-0 where -T[0] is written)


def _circuits():
    """The circuits of the rate-by-path matrix (tests/test_gpu_sample_rates.py), built at the rate configured last."""
    def four(w):
        return lambda: d.Sum.many([d.Osc(f, w) for f in (110.25, 220.5, 331.0, 441.75)])
    return {
        "fm_pair": lambda: d.Osc(d.Sum(d.Multiply(d.Osc(3), 200), 440)),
        **{"four_" + w: four(w) for w in ("sin", "saw", "square", "triangle", "8bit")},
        "osc_ramp": lambda: d.Multiply(d.Osc(440.5), d.Ramp(1000, 1, 0).trigger()),
        "osc_shape": lambda: d.Multiply(d.Osc(440.5), d.Shape("semiSine", 0.03).trigger()),
        "osc_ahd": lambda: d.Multiply(d.Osc(440.5), d.AHD(0.01, 0.02, 0.03).trigger()),
        "filter_const": lambda: d.Filter(d.Osc(150, "saw"), 3000),
        "filter_mod": lambda: d.Filter(d.Osc(150, "saw"), d.Sum(d.Multiply(d.Osc(5), 800), 1000)),
        "delay_whole": lambda: d.Delay(d.Osc(500), 300, 1024),
        "delay_frac": lambda: d.Delay(d.Osc(500), 300.5, 1024),
        "circlebuffer": cases._taps,
    }


CIRCUITS = list(_circuits())


@pytest.mark.parametrize("sr", COMPILE_RATES)
def test_circuits_compile_at_every_rate(sr):
    """Every circuit the compiler takes compiles for gfx950 at every rate up to 2^17 (hiprtc, no GPU): the half-table image stays out
    of LDS where it does not fit (88.2 kHz and up), whether the circuit has LDS scratch or not.  Above 2^17: a clean -2."""
    d.configure(sr)
    try:
        for name, build in _circuits().items():
            words = descriptor.extract(build()).words
            for waves in (16, 4):
                if sr > 131072:
                    with pytest.raises(runtime.DuspHipError) as e:
                        runtime.circuit_kernel_source(words, waves, 1, compile=True)
                    assert e.value.status == -2 and "sample rate above 2^17" in e.value.message, (name, waves)
                    continue
                try:
                    text = runtime.circuit_kernel_source(words, waves, 1, compile=True)
                except runtime.DuspHipError as e:
                    pytest.fail("%s at %d Hz, %d waves: %s" % (name, sr, waves, e))
                # (the kernel's table argument: 0 the sine image in LDS, -1 none — lookups gathered from global memory, or closed forms)
                image = "jit_begin<%d, 0," % waves in text
                assert image or "jit_begin<%d, -1," % waves in text, (name, sr, waves)
                sine = name not in ("four_saw", "four_square", "four_triangle", "filter_const")
                assert image == (sine and sr % 2 == 0 and sr < 88200), (name, sr, waves)  # (the image fits up to about 85 kHz)
    finally:
        d.configure(48000)
