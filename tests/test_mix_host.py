"""The contract of the device-side mix, on the CPU: dusp_amd.mix.mix_chain — the reference's left-deep `Sum.many` chain with one f32
rounding per add (Sum.js:18-29) — over the oracle's per-instance renders of unified voices IS the oracle's render of `Sum.many` of
the same voices as one circuit, bit for bit; with f32 gains it is `Sum.many` of Multiply(voice, g_i).  The inputs are kept
order-sensitive: a sum in f64 rounded once must differ from the chain in at least half the samples at 37 voices."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import dusp_amd as d
from dusp_amd import descriptor
from dusp_amd.mix import mix_chain
from conftest import ROOT
from mix_voices import voice

N_SAMPLES = 256 * 5 + 77
KINDS = ["filtered_saw", "feedback", "pan"]
COUNTS = [1, 2, 37]


def gains_for(n):
    return (0.05 + 1.9 * np.random.RandomState(n).random_sample(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def per_instance(kind, n, oracle):
    """the oracle's renders of the unified voices, one by one: float32 [n, channels, samples]"""
    d.configure(48000)
    uni = descriptor.unify([descriptor.extract(voice(kind, k)) for k in range(n)])
    planar = np.stack(oracle.render_instances(uni.words, N_SAMPLES, uni.params, uni.n_instances, range(n))).astype(np.float32)
    planar.setflags(write=False)
    return planar


def as_one_circuit(kind, n, oracle, gains=None):
    d.configure(48000)
    voices = [voice(kind, k) for k in range(n)]
    if gains is not None:
        voices = [d.Multiply(v, float(g)) for v, g in zip(voices, gains)]
    return np.asarray(oracle.render(descriptor.extract(d.Sum.many(voices)).words, N_SAMPLES), dtype=np.float32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", KINDS)
def test_chain_over_instances_is_sum_many(kind, n, oracle):
    planar = per_instance(kind, n, oracle)
    assert planar.shape == (n, 2 if kind == "pan" else 1, N_SAMPLES) and not np.isnan(planar).any()
    want = as_one_circuit(kind, n, oracle)
    got = mix_chain(planar)
    assert got.dtype == np.float32 and same_bits(got, want), "first differing sample %d" % int(np.argmax((got != want).any(axis=0)))
    if n == 37:  # a sum rounded once is another result: a wrong order or a tree reduction cannot pass for the chain
        once = planar.astype(np.float64).sum(axis=0).astype(np.float32)
        differing = float(np.mean(once != want))
        assert differing >= 0.5, differing


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", KINDS)
def test_chain_with_gains_is_sum_many_of_multiplies(kind, n, oracle):
    planar, gains = per_instance(kind, n, oracle), gains_for(n)
    want = as_one_circuit(kind, n, oracle, gains)
    got = mix_chain(planar, gains)
    assert same_bits(got, want), "first differing sample %d" % int(np.argmax((got != want).any(axis=0)))
    if n == 37:
        once = (planar.astype(np.float64) * gains.astype(np.float64)[:, None, None]).sum(axis=0).astype(np.float32)
        assert float(np.mean(once != want)) >= 0.5


@pytest.mark.parametrize("with_gains", [False, True])
def test_a_chain_split_anywhere_and_continued_is_the_same_chain(with_gains):
    rng = np.random.RandomState(5)
    n = 11
    planar = (rng.standard_normal((n, 2, 301)) * np.logspace(-3, 3, n)[:, None, None]).astype(np.float32)
    planar[3, 0, :4] = [-0.0, np.nan, np.inf, 0.0]
    planar[0, 1, :3] = [-0.0, -0.0, 1e-42]
    planar[1:, 1, 0] = -0.0  # a column of -0: the raw chain keeps it, the copy-out makes it +0
    gains = gains_for(n) if with_gains else None
    whole_raw, whole = mix_chain(planar, gains, raw=True), mix_chain(planar, gains)
    assert np.signbit(whole_raw[1, 0]) and whole_raw[1, 0] == 0 and not np.signbit(whole[1, 0])
    assert np.isnan(whole_raw[0, 1]) and whole[0, 1] == 0 and np.isinf(whole[0, 2])
    for cut in range(1, n):
        head = mix_chain(planar[:cut], None if gains is None else gains[:cut], raw=True)
        for raw, want in ((True, whole_raw), (False, whole)):
            got = mix_chain(planar[cut:], None if gains is None else gains[cut:], init=head, raw=raw)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), (cut, raw)
    # three pieces, and a chain that starts from init at its very first voice
    a = mix_chain(planar[:2], None if gains is None else gains[:2], raw=True)
    b = mix_chain(planar[2:7], None if gains is None else gains[2:7], init=a, raw=True)
    c = mix_chain(planar[7:], None if gains is None else gains[7:], init=b)
    assert np.array_equal(c.view(np.uint32), whole.view(np.uint32))


def test_the_chain_starts_from_the_first_voice_itself():
    x = np.array([[[-0.0, 1.0]]], dtype=np.float32)
    assert np.signbit(mix_chain(x, raw=True)[0, 0])                                           # not 0 + (-0) = +0
    assert not np.signbit(mix_chain(x, init=np.zeros((1, 2), np.float32), raw=True)[0, 0])    # ... which a chain continued from zeros is
    assert not np.signbit(mix_chain(x)[0, 0])


def test_argument_shapes_are_checked():
    x = np.zeros((3, 2, 5), dtype=np.float32)
    for bad in (lambda: mix_chain(x[0]), lambda: mix_chain(x[:0]), lambda: mix_chain(x, gains=[1, 2]), lambda: mix_chain(x, init=np.zeros((2, 4)))):
        with pytest.raises(ValueError, match="dusp-hip"):
            bad()


def test_mix_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/mix_engine.hip itself, compiled for the host with its lanes run one after the other (tests/native/hip_host_stub), under
    AddressSanitizer and UBSan: every launcher choice, gains, init, in place, raw, unaligned outputs and inputs — the contract's bits, and
    no access outside the buffers."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "mix_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w",
                           "-I", os.path.join(native, "hip_host_stub"), "-x", "c++", os.path.join(native, "mix_kernel_check.cpp"), "-o", exe])
    rep = json.loads(subprocess.check_output([exe]).decode().strip().splitlines()[-1])
    assert rep["cases"] > 3000 and rep["bad"] == 0, rep
