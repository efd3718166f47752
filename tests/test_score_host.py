"""The contract of score rendering, on the CPU: dusp_amd.mix.score_chain — voices placed at per-voice onsets on a timeline and added in
index order, one f32 rounding per add, a voice taking no part outside its span — over the oracle's per-instance renders IS the oracle's
render of `Sum.many(Delay(voice_k, onset_k, maxDelay))` as one circuit, bit for bit.  Then the chain's own algebra on planted data (cut
anywhere in the voices or in the timeline and continued through init, it is the same chain), its edge cases, and the two CPU programs
that hold the launch plan and the kernel's text to it under sanitizers."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import mix_voices
import score_voices as sv
from conftest import ROOT
from dusp_amd import descriptor
from dusp_amd.mix import mix_chain, score_chain

COUNTS = [1, 2, 13, 37]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    """bit patterns; for NaN, the positions"""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


@functools.lru_cache(maxsize=None)
def per_instance(kind, n, n_samples, oracle):
    d.configure(sv.SAMPLE_RATE)
    make = sv.voice if kind == "score" else functools.partial(mix_voices.voice, kind)
    uni = descriptor.unify([descriptor.extract(make(k)) for k in range(n)])
    planar = np.stack(oracle.render_instances(uni.words, n_samples, uni.params, uni.n_instances, range(n))).astype(np.float32)
    planar.setflags(write=False)
    return planar


def one_circuit(kind, n, oracle, gains=None):
    d.configure(sv.SAMPLE_RATE)
    make = sv.voice if kind == "score" else functools.partial(mix_voices.voice, kind)
    circuit = sv.as_one_circuit([make(k) for k in range(n)], sv.layout(n)[0], gains)
    return np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("n", COUNTS)
def test_chain_over_instances_is_sum_many_of_delays(n, with_gains, oracle):
    planar = per_instance("score", n, sv.NV, oracle)
    onsets, lengths, gains = sv.layout(n)
    assert planar.shape == (n, 1, sv.NV) and not np.isnan(planar).any()
    assert not planar[:, :, 700:].any(), "the voice's tail is not zeros: the lengths would cut sound off"
    assert (onsets + lengths > sv.NT).any() or n < 13  # (voices straddle the timeline's end)
    g = gains if with_gains else None
    want = one_circuit("score", n, oracle, g)
    got = score_chain(planar, onsets, sv.NT, lengths, g)
    assert got.dtype == np.float32 and got.shape == (1, sv.NT)
    assert np.array_equal(bits(got), bits(want)), "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0)))
    assert np.array_equal(bits(score_chain(planar, onsets, sv.NT, None, g)), bits(want))  # (what the lengths cut off is zeros)
    if n == 37:  # a sum rounded once is another result: a wrong order or a tree reduction cannot pass for the chain
        rows = np.zeros((n, sv.NT + sv.NV), dtype=np.float64)
        for k in range(n):
            rows[k, onsets[k]:onsets[k] + sv.NV] = planar[k, 0].astype(np.float64) * (np.float64(g[k]) if with_gains else 1.0)
        once = rows.sum(axis=0)[:sv.NT].astype(np.float32)
        differing = float(np.mean(once != want[0]))
        print("differing from a sum rounded once: %.3f" % differing)
        assert differing >= 0.25, differing


@pytest.mark.parametrize("n", [1, 2, 13])
@pytest.mark.parametrize("kind", ["filtered_saw", "feedback", "pan"])
def test_chain_over_the_mix_voices_is_sum_many_of_delays(kind, n, oracle):
    """voices that never end: each is rendered for the whole timeline, and no lengths clip it"""
    planar = per_instance(kind, n, sv.NT, oracle)
    want = one_circuit(kind, n, oracle)
    got = score_chain(planar, sv.layout(n)[0], sv.NT)
    assert got.shape == (2 if kind == "pan" else 1, sv.NT)
    assert np.array_equal(bits(got), bits(want)), "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0)))


def planted(n=11, n_ch=2, n_voice=97, n_total=301):
    rng = np.random.RandomState(5)
    planar = (rng.standard_normal((n, n_ch, n_voice)) * np.logspace(-3, 3, n)[:, None, None]).astype(np.float32)
    planar[3, 0, :4] = [-0.0, np.nan, np.inf, 0.0]
    planar[0, 1, :3] = [-0.0, -0.0, 1e-42]
    planar[:, 1, 40] = -0.0
    onsets = rng.randint(-n_voice + 1, n_total, n).astype(np.int64)
    onsets[3], onsets[0], onsets[5], onsets[6] = 10, 200, -30, n_total - 20
    lengths = rng.randint(0, n_voice + 1, n).astype(np.int64)
    lengths[[0, 3, 5, 6]] = n_voice
    gains = (0.05 + 1.9 * rng.random_sample(n)).astype(np.float32)
    gains[1] = -gains[1]
    return planar, onsets, lengths, gains, n_total


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
def test_a_chain_cut_anywhere_in_the_voices_and_continued_is_the_same_chain(with_gains):
    planar, onsets, lengths, gains, n_total = planted()
    n = len(onsets)
    g = gains if with_gains else None
    whole_raw, whole = score_chain(planar, onsets, n_total, lengths, g, raw=True), score_chain(planar, onsets, n_total, lengths, g)
    assert np.isnan(whole_raw[0, 11]) and whole[0, 11] == 0 and not np.signbit(whole[0, 11]) and np.isinf(whole[0, 12])
    for cut in range(0, n + 1):
        head = score_chain(planar[:cut], onsets[:cut], n_total, lengths[:cut], None if g is None else g[:cut], raw=True)
        for raw, want in ((True, whole_raw), (False, whole)):
            got = score_chain(planar[cut:], onsets[cut:], n_total, lengths[cut:], None if g is None else g[cut:], init=head, raw=raw)
            assert same(got, want), (cut, raw)
    # a -0 partial sum survives voices that do not cover the sample (nothing is added there, not even a zero) ...
    init = np.full((2, n_total), -0.0, dtype=np.float32)
    uncovered = np.ones(n_total, dtype=bool)
    for k in range(n):
        uncovered[max(int(onsets[k]), 0):max(int(onsets[k] + lengths[k]), 0)] = False
    assert uncovered.any()
    cont = score_chain(planar, onsets, n_total, lengths, g, init=init, raw=True)
    assert np.signbit(cont[:, uncovered]).all() and (cont[:, uncovered] == 0).all()
    assert not np.signbit(score_chain(planar, onsets, n_total, lengths, g, init=init)[:, uncovered]).any()  # ... and leaves as +0


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
def test_the_timeline_cut_into_two_windows_is_the_whole(with_gains):
    planar, onsets, lengths, gains, n_total = planted()
    g = gains if with_gains else None
    for raw in (True, False):
        whole = score_chain(planar, onsets, n_total, lengths, g, raw=raw)
        for cut in (1, 100, 128, 199, 300):
            first = score_chain(planar, onsets, cut, lengths, g, raw=raw)
            second = score_chain(planar, onsets - cut, n_total - cut, lengths, g, raw=raw)  # (onsets shifted: many are negative now)
            assert same(np.concatenate([first, second], axis=1), whole), (raw, cut)


def test_onsets_all_zero_and_full_lengths_is_the_mix():
    planar = planted()[0]
    n, _, n_voice = planar.shape
    gains = planted()[3]
    zeros = np.zeros(n, dtype=np.int64)
    assert same(score_chain(planar, zeros, n_voice), mix_chain(planar))
    assert same(score_chain(planar, zeros, n_voice, gains=gains), mix_chain(planar, gains))
    assert same(score_chain(planar, zeros, n_voice, np.full(n, n_voice)), mix_chain(planar))
    # raw, the two differ in the sign of a zero only: the score's chain starts from +0, the mix's from the first voice itself
    a, b = score_chain(planar, zeros, n_voice, raw=True), mix_chain(planar, raw=True)
    differ = bits(a) != bits(b)
    assert differ.any() and (a[differ & ~np.isnan(a)] == 0).all() and (b[differ & ~np.isnan(b)] == 0).all()


def test_planted_edge_cases():
    f = lambda *rows: np.array(rows, dtype=np.float32)[:, None, :]  # voices of one channel
    x = f([1, 2, 3], [10, 20, 30])
    chain = lambda *a, **kw: score_chain(*a, **kw)[0].tolist()
    assert chain(x, [0, 0], 5) == [11, 22, 33, 0, 0]                       # two voices at one onset
    assert chain(x, [-1, -2], 5) == [32, 3, 0, 0, 0]                       # negative onsets: the voices began before the timeline
    assert chain(x, [-3, -100], 5) == [0, 0, 0, 0, 0]                      # ... wholly before it
    assert chain(x, [5, 6], 5) == [0, 0, 0, 0, 0]                          # onsets past the end
    assert chain(x, [3, 4], 5) == [0, 0, 0, 1, 12]                         # voices straddling the end
    assert chain(x, [0, 1], 5, [0, 1]) == [0, 10, 0, 0, 0]                 # len = 0 and len = 1
    assert chain(x, [2 ** 62, -2 ** 62], 5) == [0, 0, 0, 0, 0]             # far out on both sides
    assert chain(x, [np.iinfo(np.int64).max, np.iinfo(np.int64).min], 5) == [0, 0, 0, 0, 0]
    init = f([7, 8, 9, -0.0, 5])[0]
    got = score_chain(x, [0, 0], 5, [1, 1], init=init, raw=True)[0]
    assert got.tolist() == [18, 8, 9, 0, 5] and np.signbit(got[3])          # a sample no voice covers is init, its -0 included
    assert not np.signbit(score_chain(x, [0, 0], 5, [1, 1], init=init)[0][3])
    none = score_chain(x, [9, 9], 5, raw=True)
    assert not none.any() and not np.signbit(none).any()                    # ... or +0
    z = f([-0.0, -0.0])
    alone = score_chain(z, [1], 4, raw=True)[0]
    assert (alone == 0).all() and not np.signbit(alone).any()               # a -0 sample alone: +0 + -0 = +0
    assert np.signbit(mix_chain(z, raw=True)).all()                         # (where the mix's chain keeps it)
    assert score_chain(np.zeros((0, 2, 3), np.float32), [], 4).shape == (2, 4)  # no voices: the timeline of +0
    g = score_chain(x, [0, 1], 4, gains=[2, -1])[0]
    assert g.tolist() == [2, -6, -14, -30]
    assert chain(x, np.array([1.0, 0.0]), 4) == [10, 21, 32, 3]            # whole numbers may come as floats


def test_argument_shapes_are_checked():
    x = np.zeros((3, 2, 5), dtype=np.float32)
    on = [0, 1, 2]
    for bad in (lambda: score_chain(x[0], on, 9), lambda: score_chain(x, [0, 1], 9), lambda: score_chain(x, on, 9, lengths=[1, 2]),
                lambda: score_chain(x, on, 9, lengths=[1, 2, 6]), lambda: score_chain(x, on, 9, lengths=[1, -1, 2]), lambda: score_chain(x, on, 9, gains=[1, 2]),
                lambda: score_chain(x, on, 9, init=np.zeros((2, 5))), lambda: score_chain(x, [0, 0.5, 1], 9), lambda: score_chain(x, on, 9, lengths=[1, 1.5, 2]),
                lambda: score_chain(x, on, -1), lambda: score_chain(x, on, 2.5), lambda: score_chain(x, [0, np.nan, 1], 9)):
        with pytest.raises(ValueError, match="dusp-hip"):
            bad()


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_score_plan_against_brute_force_under_sanitizers(tmp_path):
    """dusp_amd/csrc/score_plan.hpp: every block's list is the ascending set of intersecting voices, the union window, onsets near
    +-2^62 and at the int64 limits, and the byte budget honoured by doubling the block (tests/native/score_plan_check.cpp)."""
    exe = str(tmp_path / "score_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + SANITIZE + [os.path.join(ROOT, "tests", "native", "score_plan_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] >= 5000 and rep["doubled"] >= 100 and rep["far_onsets"] >= 1000 and rep["empty_tiles"] >= 10, rep


def test_score_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/score_engine.hip itself, compiled for the host with its lanes run one after the other (tests/native/hip_host_stub), fed
    score_plan.hpp's plans, under AddressSanitizer and UBSan: the contract's bits and no access outside the buffers
    (tests/native/score_kernel_check.cpp lists what it covers)."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "score_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub"), "-x", "c++",
                           os.path.join(native, "score_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 10000 and rep["doubled"] >= 100 and rep["windows"] >= 100, rep
