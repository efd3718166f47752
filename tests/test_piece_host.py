"""Pieces of several instruments, on the CPU: dusp_amd.mix.score_chain_rows — score_chain over voices that are rows of their own lengths —
over the oracle's per-part renders IS the oracle's render of `Sum.many(Delay(voice_k, onset_k, maxDelay))` over the interleaved voice
list as one circuit, bit for bit.  Then the chain's algebra on planted rows of mixed lengths, the grouping of a voice list into parts
(render.piece_parts), and the two CPU programs that hold the rows plan and the rows kernel's text to the contract under sanitizers."""
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
from dusp_amd import descriptor, render, runtime
from dusp_amd.mix import score_chain, score_chain_rows

NV_SAW = 1031  # samples a filtered-saw voice is rendered for (the score voice: sv.NV = 773)
FMAX = np.finfo(np.float32).max
PLANTED = [0.0, -0.0, np.inf, -np.inf, FMAX, -FMAX, 1e-45, -1e-40, 5e-39, 1.0, -1.0, np.nan]  # (test_gpu_score.py's)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    """bit patterns; for NaN, the positions"""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def saw_voice(k):
    """the second structure: mix_voices' filtered saw as a NOTE — under a Ramp that has ended by sample 1000, so that what lies behind the
    1031 samples it is rendered for is zeros, as behind the score voice's 773 (a piece's voice ends; the bare saw never would)"""
    return d.Multiply(mix_voices.voice("filtered_saw", k), d.Ramp(1000, 1, 0).trigger())


def interleaved_voice(k):
    """voice k of the piece: the score voice and the filtered saw in turn, each counted on its own"""
    return sv.voice(k // 2) if k % 2 == 0 else saw_voice(k // 2)


@functools.lru_cache(maxsize=None)
def oracle_rows(n, oracle):
    """the oracle's render of every voice of the interleaved list, PART BY PART (each part unified and rendered for its own length)"""
    d.configure(sv.SAMPLE_RATE)
    grouped = render.piece_parts([descriptor.extract(interleaved_voice(k)) for k in range(n)], [sv.NV if k % 2 == 0 else NV_SAW for k in range(n)])
    per_part = [np.stack(oracle.render_instances(uni.words, n_voice, uni.params, uni.n_instances, range(uni.n_instances))).astype(np.float32) for uni, n_voice in grouped.parts]
    rows = [per_part[p][i] for p, i in zip(grouped.part_of, grouped.instance_of)]
    for r in rows:
        r.setflags(write=False)
    return rows


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("n", [2, 13, 37])
def test_chain_over_the_parts_renders_is_sum_many_of_delays_over_the_interleaved_list(n, with_gains, oracle):
    rows = oracle_rows(n, oracle)
    assert [r.shape for r in rows] == [(1, sv.NV if k % 2 == 0 else NV_SAW) for k in range(n)] and not np.isnan(np.concatenate(rows, axis=1)).any()
    assert not any(r[:, 1000:].any() for r in rows[1::2]) and any(r[:, 900:1000].any() for r in rows[1::2]), "the saw voice's tail is not zeros behind its Ramp"
    onsets, _, gains = sv.layout(n)
    assert (onsets == 0).sum() == 1 and (n < 3 or (gains < 0).sum() == 1)
    g = gains if with_gains else None
    d.configure(sv.SAMPLE_RATE)
    circuit = sv.as_one_circuit([interleaved_voice(k) for k in range(n)], onsets, g)
    want = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
    got = score_chain_rows(rows, onsets, sv.NT, None, g)
    assert got.dtype == np.float32 and got.shape == (1, sv.NT)
    assert np.array_equal(bits(got), bits(want)), "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0)))


def planted_rows(n_ch=2, n_total=1301):
    """rows of 1, 255, 257 and 773 samples mixed in one list, with the planted values among them"""
    rng = np.random.RandomState(7)
    samples = [773, 1, 255, 257, 1, 773, 257, 255, 773, 1, 257]
    n = len(samples)
    rows = [(rng.standard_normal((n_ch, s)) * 10.0 ** (k % 7 - 3)).astype(np.float32) for k, s in enumerate(samples)]
    big = [k for k, s in enumerate(samples) if s >= 255]
    for j, v in enumerate(PLANTED):
        rows[big[j % len(big)]][j % n_ch, 3 + j] = v
    rows[1][:, 0] = -0.0
    rows[3][0, :4] = [-0.0, np.nan, np.inf, 0.0]
    onsets = rng.randint(-200, n_total, n).astype(np.int64)
    onsets[3], onsets[0], onsets[5], onsets[8], onsets[1] = 10, 900, -300, n_total - 20, 12
    lengths = np.array([rng.randint(0, s + 1) for s in samples], dtype=np.int64)
    lengths[[0, 1, 3, 5, 8]] = [samples[k] for k in (0, 1, 3, 5, 8)]
    gains = (0.05 + 1.9 * rng.random_sample(n)).astype(np.float32)
    gains[1] = -gains[1]
    return rows, onsets, lengths, gains, n_total


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
def test_a_chain_of_rows_cut_at_every_voice_and_continued_is_the_same_chain(with_gains):
    rows, onsets, lengths, gains, n_total = planted_rows()
    n = len(rows)
    g = gains if with_gains else None
    whole_raw, whole = score_chain_rows(rows, onsets, n_total, lengths, g, raw=True), score_chain_rows(rows, onsets, n_total, lengths, g)
    assert np.isnan(whole_raw).any() and not np.isnan(whole).any() and np.isinf(whole).any()
    for cut in range(0, n + 1):
        head = score_chain_rows(rows[:cut], onsets[:cut], n_total, lengths[:cut], None if g is None else g[:cut], raw=True) if cut else np.zeros((2, n_total), dtype=np.float32)
        for raw, want in ((True, whole_raw), (False, whole)):
            got = score_chain_rows(rows[cut:], onsets[cut:], n_total, lengths[cut:], None if g is None else g[cut:], init=head, raw=raw)
            assert same(got, want), (cut, raw)
    # a -0 partial sum survives voices that do not cover the sample, and leaves as +0
    uncovered = np.ones(n_total, dtype=bool)
    for k in range(n):
        uncovered[max(int(onsets[k]), 0):max(int(onsets[k] + lengths[k]), 0)] = False
    assert uncovered.any()
    init = np.full((2, n_total), -0.0, dtype=np.float32)
    cont = score_chain_rows(rows, onsets, n_total, lengths, g, init=init, raw=True)
    assert np.signbit(cont[:, uncovered]).all() and (cont[:, uncovered] == 0).all()
    assert not np.signbit(score_chain_rows(rows, onsets, n_total, lengths, g, init=init)[:, uncovered]).any()


@pytest.mark.parametrize("with_gains", [False, True], ids=["plain", "gains"])
def test_the_timeline_of_rows_cut_into_windows_is_the_whole(with_gains):
    rows, onsets, lengths, gains, n_total = planted_rows()
    g = gains if with_gains else None
    for raw in (True, False):
        whole = score_chain_rows(rows, onsets, n_total, lengths, g, raw=raw)
        for cut in (1, 13, 256, 899, 1300):
            first = score_chain_rows(rows, onsets, cut, lengths, g, raw=raw)
            second = score_chain_rows(rows, onsets - cut, n_total - cut, lengths, g, raw=raw)  # (onsets shifted: many are negative now)
            assert same(np.concatenate([first, second], axis=1), whole), (raw, cut)


def test_rows_of_one_length_are_score_chain_of_their_stack():
    rng = np.random.RandomState(3)
    planar = (rng.standard_normal((9, 2, 97)) * np.logspace(-3, 3, 9)[:, None, None]).astype(np.float32)
    planar[2, 0, :3] = [-0.0, np.nan, np.inf]
    onsets = rng.randint(-96, 301, 9).astype(np.int64)
    lengths = rng.randint(0, 98, 9).astype(np.int64)
    gains = (0.05 + 1.9 * rng.random_sample(9)).astype(np.float32)
    init = (30 * rng.standard_normal((2, 301))).astype(np.float32)
    init[0, 5] = -0.0
    for kw in ({}, {"lengths": lengths}, {"gains": gains}, {"lengths": lengths, "gains": gains, "init": init}, {"init": init, "raw": True}, {"lengths": lengths, "raw": True}):
        assert same(score_chain_rows(list(planar), onsets, 301, **kw), score_chain(planar, onsets, 301, **kw)), sorted(kw)
    assert score_chain_rows([], [], 4).shape == (1, 4) and not score_chain_rows([], [], 4).any()
    assert same(score_chain_rows([], [], 301, init=init), score_chain(np.zeros((0, 2, 5), np.float32), [], 301, init=init))


def test_rows_argument_shapes_are_checked():
    a, b = np.zeros((2, 5), np.float32), np.zeros((2, 3), np.float32)
    for bad in (lambda: score_chain_rows([a, np.zeros((1, 3), np.float32)], [0, 1], 9), lambda: score_chain_rows([a, np.zeros(3, np.float32)], [0, 1], 9),
                lambda: score_chain_rows([a, b], [0], 9), lambda: score_chain_rows([a, b], [0, 1], 9, lengths=[5, 4]), lambda: score_chain_rows([a, b], [0, 1], 9, lengths=[-1, 3]),
                lambda: score_chain_rows([a, b], [0, 1], 9, gains=[1]), lambda: score_chain_rows([a, b], [0, 1], 9, init=np.zeros((2, 8))),
                lambda: score_chain_rows([a, b], [0, 0.5], 9), lambda: score_chain_rows([a, b], [0, 1], -1)):
        with pytest.raises(ValueError, match="dusp-hip"):
            bad()
    assert score_chain_rows([a, b], [0, 1], 9, lengths=[5, 3]).shape == (2, 9)


# ---- grouping a voice list into parts ----------------------------------------------------------------------------------------------

def test_a_mixed_voice_list_is_grouped_into_parts_by_structure_and_length():
    d.configure(sv.SAMPLE_RATE)
    kinds = ["score", "saw", "score", "pan", "saw", "score", "saw", "score"]
    samples = [773, 1031, 773, 500, 1031, 400, 1031, 773]  # (voice 5: the score voice's structure, but another length: a part of its own)
    made = {"score": 0, "saw": 0, "pan": 0}
    voices = []
    for kind in kinds:
        k = made[kind]
        made[kind] += 1
        voices.append(sv.voice(k) if kind == "score" else mix_voices.voice("filtered_saw" if kind == "saw" else "pan", k))
    extractions = [descriptor.extract(v) for v in voices]
    grouped = render.piece_parts(extractions, samples)
    assert grouped.part_of.tolist() == [0, 1, 0, 2, 1, 3, 1, 0] and grouped.instance_of.tolist() == [0, 0, 1, 0, 1, 0, 2, 2]
    assert [(uni.n_instances, n) for uni, n in grouped.parts] == [(3, 773), (3, 1031), (1, 500), (1, 400)] and grouped.sample_rate == sv.SAMPLE_RATE
    # every part is the unify of its own voices, in their order in the list
    for p, (uni, _) in enumerate(grouped.parts):
        mine = descriptor.unify([e for e, q in zip(extractions, grouped.part_of) if q == p])
        assert np.array_equal(uni.words, mine.words, equal_nan=True) and (uni.params is None) == (mine.params is None)
        assert uni.params is None or np.array_equal(uni.params, mine.params)
    # the next unused instance of a voice's part is that voice's instance
    used = [0] * len(grouped.parts)
    for p, i in zip(grouped.part_of, grouped.instance_of):
        assert used[p] == i
        used[p] += 1
    # what unify takes as one program has one key; what it refuses has another
    keys = [render.structure_key(e) for e in extractions]
    assert keys[0] == keys[2] == keys[5] and keys[1] == keys[4] and len({keys[0], keys[1], keys[3]}) == 3
    with pytest.raises(descriptor.DuspError, match="differs"):
        descriptor.unify([extractions[0], extractions[1]])
    with pytest.raises(descriptor.DuspError, match="dusp-hip: no instances"):
        render.piece_parts([], [])


def test_parts_of_different_channel_counts_are_refused_by_string():
    """... before anything is built: the channel count comes from the descriptor, on the host (dusp_descriptor_channels)"""
    d.configure(sv.SAMPLE_RATE)
    assert runtime.descriptor_channels(descriptor.extract(sv.voice(0)).words) == 1
    assert runtime.descriptor_channels(descriptor.extract(mix_voices.voice("pan", 0)).words) == 2
    with pytest.raises(runtime.DuspHipError, match="dusp_descriptor_channels"):
        runtime.descriptor_channels(np.zeros(5))
    assert render.check_piece_channels([2, 2, 2]) == 2
    with pytest.raises(descriptor.DuspError, match="dusp-hip: the voices of a piece must have one number of output channels: part 1 has 2, part 0 has 1"):
        render.check_piece_channels([1, 2, 1])
    voices = lambda: [sv.voice(0), mix_voices.voice("pan", 0), sv.voice(1)]
    for call in (lambda: d.render_piece(voices(), [0, 1, 2], 0.01, 0.05), lambda: d.render_piece_pcm(voices(), [0, 1, 2], [0.01, 0.02, 0.01], 0.05),
                 lambda: d.render_piece_wav(voices(), [0, 1, 2], 0.01, 0)):
        with pytest.raises(descriptor.DuspError, match="one number of output channels: part 1 has 2, part 0 has 1"):
            call()
    # the other refusals that need no device
    for call, needle in [(lambda: d.render_piece(voices()[::2], [0, 0.5], 0.01, 0.05), "whole numbers"), (lambda: d.render_piece(voices()[::2], [0], 0.01, 0.05), "onsets must have shape"),
                         (lambda: d.render_piece(voices()[::2], [0, 1], [0.01], 0.05), "voice_durations must be one number or have shape"),
                         (lambda: d.render_piece(voices()[::2], [0, 1], [0.01, 0.02], 0.05, lengths=[480, 961]), "lengths must lie in 0 .. the voice's own samples"),
                         (lambda: d.render_piece(voices()[::2], [0, 1], 0.01, 0.05, gains=[1.0]), "gains must have shape")]:
        with pytest.raises(ValueError, match=needle):
            call()
    with pytest.raises(descriptor.DuspError, match="voice_duration must cover at least one sample"):
        d.render_piece(voices()[::2], [0, 1], [0.01, 0], 0.05)


# ---- the plan and the kernel's text, under sanitizers ------------------------------------------------------------------------------

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_score_rows_plan_against_brute_force_under_sanitizers(tmp_path):
    """score_rows_plan of dusp_amd/csrc/score_plan.hpp (tests/native/score_rows_plan_check.cpp lists what it covers)"""
    exe = str(tmp_path / "score_rows_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + SANITIZE + [os.path.join(ROOT, "tests", "native", "score_rows_plan_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] >= 5000 and rep["doubled"] >= 100 and rep["far_onsets"] >= 1000 and rep["empty_tiles"] >= 10 and rep["empty_rows"] >= 1000, rep


def test_score_rows_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/score_rows_engine.hip itself, compiled for the host with its lanes run one after the other, every row a heap
    allocation of exactly its size, under AddressSanitizer and UBSan (tests/native/score_rows_kernel_check.cpp lists what it covers)."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "score_rows_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub"), "-x", "c++",
                           os.path.join(native, "score_rows_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 5000 and rep["doubled"] >= 100 and rep["windows"] >= 100 and rep["zero_first"] >= 1000, rep
