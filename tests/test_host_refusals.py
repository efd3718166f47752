"""Every refusal of the Python host that needs no device, by exception type and full message: the numpy contracts of dusp_amd.mix, the
argument helpers of dusp_amd.runtime, and what dusp_amd.render refuses before a context is made.  The strings are the record of what
the host says (the JavaScript host is compared with them in test_pan_host.py and test_frac_host.py); where a call has two bad arguments
the table pins which one is named, that is the order of the checks."""
import numpy as np
import pytest

import dusp_amd as d
import mix_voices
import score_voices as sv
from dusp_amd import mix, render, runtime
from dusp_amd.descriptor import DuspError

F32 = np.float32
P = np.zeros((2, 1, 24), F32)                         # two voices of one channel, planar
A, B, C = np.zeros((1, 24), F32), np.zeros((1, 17), F32), np.zeros((2, 17), F32)  # rows: mono, mono, two channels
SHORT, LONG = 0.001, 0.002                            # seconds: 48 and 96 samples at 48 kHz


def mono():
    return [sv.voice(0), sv.voice(1), sv.voice(2)]


def two_structures():
    return [sv.voice(0), mix_voices.voice("filtered_saw", 0), sv.voice(1)]


def two_channel_counts():
    return [sv.voice(0), mix_voices.voice("pan", 0), sv.voice(1)]


V, W = "ValueError", "DuspError"
WHOLE = "dusp-hip: %s are whole numbers of samples"
IN_SAMPLES = "dusp-hip: %s are in samples, whole numbers: a fraction (or what is no number) is refused"
N_TOTAL = "dusp-hip: n_total must be a whole number of samples, not negative"
ROW_LENGTH = "dusp-hip: the length of voice %d is %d: lengths must lie in 0 .. the row's samples (%d)"
BIT_DEPTH = "dusp-hip: bit depth must be 16, 24 or 32"
NORMALISE = "dusp-hip: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale)"
NO_SAMPLES = "dusp-hip: voice_duration must cover at least one sample"
ONE_NUMBER = "dusp-hip: voice_duration is one number"
ONE_PART = "dusp-hip: the voices of a score are isomorphic circuits: a piece renders several instruments"
NOT_MONO = "dusp-hip: a panned voice is mono: part 1 has 2 output channels"
CHANNELS = "dusp-hip: the voices of a piece must have one number of output channels: part 1 has 2, part 0 has 1"

# (id, call, exception, message); "a+b" in an id: both are wrong, and the message says which is found first
CASES = [
    # ---- mix.mix_chain
    ("mix_chain planar", lambda: mix.mix_chain(np.zeros((2, 24))), V, "dusp-hip: planar must have shape (instances >= 1, channels, samples)"),
    ("mix_chain no instances", lambda: mix.mix_chain(np.zeros((0, 1, 24))), V, "dusp-hip: planar must have shape (instances >= 1, channels, samples)"),
    ("mix_chain gains", lambda: mix.mix_chain(P, gains=[1]), V, "dusp-hip: gains must have shape (instances=2,)"),
    ("mix_chain init", lambda: mix.mix_chain(P, init=np.zeros((1, 23))), V, "dusp-hip: init must have shape (channels=1, samples=24)"),
    ("mix_chain gains+init", lambda: mix.mix_chain(P, gains=[1, 2, 3], init=np.zeros(24)), V, "dusp-hip: gains must have shape (instances=2,)"),
    # ---- mix.score_chain
    ("score_chain planar", lambda: mix.score_chain(np.zeros((2, 24)), [0, 1], 30), V, "dusp-hip: planar must have shape (instances, channels, samples)"),
    ("score_chain n_total negative", lambda: mix.score_chain(P, [0, 1], -1), V, N_TOTAL),
    ("score_chain n_total fraction", lambda: mix.score_chain(P, [0, 1], 30.5), V, N_TOTAL),
    ("score_chain onsets shape", lambda: mix.score_chain(P, [0], 30), V, "dusp-hip: onsets must have shape (instances=2,)"),
    ("score_chain onsets fraction", lambda: mix.score_chain(P, [0, 0.5], 30), V, WHOLE % "onsets"),
    ("score_chain onsets nan", lambda: mix.score_chain(P, [0, np.nan], 30), V, WHOLE % "onsets"),
    ("score_chain onsets 2^63", lambda: mix.score_chain(P, [0, 2.0 ** 63], 30), V, WHOLE % "onsets"),
    ("score_chain onsets no number", lambda: mix.score_chain(P, ["0", "1"], 30), V, WHOLE % "onsets"),
    ("score_chain lengths shape", lambda: mix.score_chain(P, [0, 1], 30, lengths=[[24, 24]]), V, "dusp-hip: lengths must have shape (instances=2,)"),
    ("score_chain lengths fraction", lambda: mix.score_chain(P, [0, 1], 30, lengths=[24, 1.5]), V, WHOLE % "lengths"),
    ("score_chain lengths negative", lambda: mix.score_chain(P, [0, 1], 30, lengths=[24, -1]), V, "dusp-hip: lengths must lie in 0 .. samples=24"),
    ("score_chain lengths long", lambda: mix.score_chain(P, [0, 1], 30, lengths=[25, 0]), V, "dusp-hip: lengths must lie in 0 .. samples=24"),
    ("score_chain gains", lambda: mix.score_chain(P, [0, 1], 30, gains=[1, 2, 3]), V, "dusp-hip: gains must have shape (instances=2,)"),
    ("score_chain init", lambda: mix.score_chain(P, [0, 1], 30, init=np.zeros((1, 31))), V, "dusp-hip: init must have shape (channels=1, n_total=30)"),
    ("score_chain planar+n_total", lambda: mix.score_chain(np.zeros(24), [0], -1), V, "dusp-hip: planar must have shape (instances, channels, samples)"),
    ("score_chain n_total+onsets", lambda: mix.score_chain(P, [0], -1), V, N_TOTAL),
    ("score_chain onsets+lengths", lambda: mix.score_chain(P, [0, 0.5], 30, lengths=[99, 99]), V, WHOLE % "onsets"),
    ("score_chain lengths+gains", lambda: mix.score_chain(P, [0, 1], 30, lengths=[25, 24], gains=[1]), V, "dusp-hip: lengths must lie in 0 .. samples=24"),
    ("score_chain gains+init", lambda: mix.score_chain(P, [0, 1], 30, gains=[1], init=np.zeros(30)), V, "dusp-hip: gains must have shape (instances=2,)"),
    # ---- mix.score_chain_rows
    ("rows row shape", lambda: mix.score_chain_rows([A, np.zeros(17, F32)], [0, 1], 30), V, "dusp-hip: every row must have shape (channels, samples)"),
    ("rows n_total negative", lambda: mix.score_chain_rows([A, B], [0, 1], -1), V, N_TOTAL),
    ("rows n_total fraction", lambda: mix.score_chain_rows([A, B], [0, 1], 0.5), V, N_TOTAL),
    ("rows channels", lambda: mix.score_chain_rows([A, C], [0, 1], 30), V, "dusp-hip: every row must have the same number of channels (1)"),
    ("rows onsets shape", lambda: mix.score_chain_rows([A, B], [0, 1, 2], 30), V, "dusp-hip: onsets must have shape (voices=2,)"),
    ("rows onsets fraction", lambda: mix.score_chain_rows([A, B], [0, 0.5], 30), V, WHOLE % "onsets"),
    ("rows onsets inf", lambda: mix.score_chain_rows([A, B], [0, np.inf], 30), V, WHOLE % "onsets"),
    ("rows lengths shape", lambda: mix.score_chain_rows([A, B], [0, 1], 30, lengths=[24]), V, "dusp-hip: lengths must have shape (voices=2,)"),
    ("rows lengths fraction", lambda: mix.score_chain_rows([A, B], [0, 1], 30, lengths=[24, 16.5]), V, WHOLE % "lengths"),
    ("rows lengths long", lambda: mix.score_chain_rows([A, B], [0, 1], 30, lengths=[24, 18]), V, ROW_LENGTH % (1, 18, 17)),
    ("rows lengths negative", lambda: mix.score_chain_rows([A, B], [0, 1], 30, lengths=[-3, 18]), V, ROW_LENGTH % (0, -3, 24)),
    ("rows gains", lambda: mix.score_chain_rows([A, B], [0, 1], 30, gains=[1]), V, "dusp-hip: gains must have shape (voices=2,)"),
    ("rows fracs shape", lambda: mix.score_chain_rows([A, B], [0, 1], 30, fracs=[0.5]), V, "dusp-hip: fracs must have shape (voices=2,)"),
    ("rows fracs nan", lambda: mix.score_chain_rows([A, B], [0, 1], 30, fracs=[0, np.nan]), V, "dusp-hip: the fraction of voice 1 is not finite"),
    ("rows fracs one", lambda: mix.score_chain_rows([A, B], [0, 1], 30, fracs=[1.0, 0]), V, "dusp-hip: the fraction of voice 0 is outside [0, 1)"),
    ("rows init", lambda: mix.score_chain_rows([A, B], [0, 1], 30, init=np.zeros((2, 30))), V, "dusp-hip: init must have shape (channels=1, n_total=30)"),
    ("rows no voices, init of one axis", lambda: mix.score_chain_rows([], [], 30, init=np.zeros(30)), V, "dusp-hip: init must have shape (channels=0, n_total=30)"),
    ("rows row shape+n_total", lambda: mix.score_chain_rows([np.zeros(17, F32)], [0], -1), V, "dusp-hip: every row must have shape (channels, samples)"),
    ("rows n_total+channels", lambda: mix.score_chain_rows([A, C], [0, 1], -1), V, N_TOTAL),
    ("rows channels+onsets", lambda: mix.score_chain_rows([A, C], [0], 30), V, "dusp-hip: every row must have the same number of channels (1)"),
    ("rows onsets+lengths", lambda: mix.score_chain_rows([A, B], [0], 30, lengths=[99, 99]), V, "dusp-hip: onsets must have shape (voices=2,)"),
    ("rows lengths+gains", lambda: mix.score_chain_rows([A, B], [0, 1], 30, lengths=[25, 18], gains=[1]), V, ROW_LENGTH % (0, 25, 24)),
    ("rows gains+fracs", lambda: mix.score_chain_rows([A, B], [0, 1], 30, gains=[1], fracs=[2, 2]), V, "dusp-hip: gains must have shape (voices=2,)"),
    ("rows fracs+init", lambda: mix.score_chain_rows([A, B], [0, 1], 30, fracs=[0, -0.5], init=np.zeros(30)), V, "dusp-hip: the fraction of voice 1 is outside [0, 1)"),
    # ---- mix.score_chain_rows_panned
    ("panned two channels", lambda: mix.score_chain_rows_panned([A, C], [0, 1], [0, 0], 30), V, "dusp-hip: every panned row must be mono, of shape (1, samples)"),
    ("panned row shape", lambda: mix.score_chain_rows_panned([A, np.zeros(17, F32)], [0, 1], [0, 0], 30), V, "dusp-hip: every panned row must be mono, of shape (1, samples)"),
    ("panned n_total", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], -1), V, N_TOTAL),
    ("panned onsets shape", lambda: mix.score_chain_rows_panned([A, B], [0], [0, 0], 30), V, "dusp-hip: onsets must have shape (voices=2,)"),
    ("panned onsets fraction", lambda: mix.score_chain_rows_panned([A, B], [0, 0.5], [0, 0], 30), V, WHOLE % "onsets"),
    ("panned pans shape", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0], 30), V, "dusp-hip: pans must have shape (voices=2,)"),
    ("panned pans nan", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, np.nan], 30), V, "dusp-hip: pans must be finite"),
    ("panned pans beyond f32", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [1e39, 0], 30), V, "dusp-hip: pans must be finite"),
    ("panned comp", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, comp=[1.0]), V, "dusp-hip: comp must have shape (voices=2,)"),
    ("panned lengths shape", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, lengths=[24, 17, 1]), V, "dusp-hip: lengths must have shape (voices=2,)"),
    ("panned lengths fraction", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, lengths=[0.5, 17]), V, WHOLE % "lengths"),
    ("panned lengths long", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, lengths=[24, 18]), V, ROW_LENGTH % (1, 18, 17)),
    ("panned gains", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, gains=[1]), V, "dusp-hip: gains must have shape (voices=2,)"),
    ("panned fracs shape", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, fracs=[0.5]), V, "dusp-hip: fracs must have shape (voices=2,)"),
    ("panned fracs inf", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, fracs=[np.inf, 0]), V, "dusp-hip: the fraction of voice 0 is not finite"),
    ("panned fracs negative", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, fracs=[0, -2.0 ** -60]), V, "dusp-hip: the fraction of voice 1 is outside [0, 1)"),
    ("panned init", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, init=np.zeros((1, 30))), V, "dusp-hip: init must have shape (channels=2, n_total=30)"),
    ("panned mono+n_total", lambda: mix.score_chain_rows_panned([C], [0], [0], -1), V, "dusp-hip: every panned row must be mono, of shape (1, samples)"),
    ("panned n_total+onsets", lambda: mix.score_chain_rows_panned([A, B], [0], [0, 0], -1), V, N_TOTAL),
    ("panned onsets+pans", lambda: mix.score_chain_rows_panned([A, B], [0, 0.5], [0], 30), V, WHOLE % "onsets"),
    ("panned pans+comp", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, np.inf], 30, comp=[1.0]), V, "dusp-hip: pans must be finite"),
    ("panned comp+lengths", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, lengths=[99, 99], comp=[1.0]), V, "dusp-hip: comp must have shape (voices=2,)"),
    ("panned lengths+gains", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, lengths=[24, -1], gains=[1]), V, ROW_LENGTH % (1, -1, 17)),
    ("panned gains+fracs", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, gains=[1], fracs=[2, 2]), V, "dusp-hip: gains must have shape (voices=2,)"),
    ("panned fracs+init", lambda: mix.score_chain_rows_panned([A, B], [0, 1], [0, 0], 30, fracs=[0, 1.5], init=np.zeros(30)), V, "dusp-hip: the fraction of voice 1 is outside [0, 1)"),
    # ---- mix.check_fracs, mix.split_onsets
    ("check_fracs shape", lambda: mix.check_fracs([0, 0], 3), V, "dusp-hip: fracs must have shape (voices=3,)"),
    ("check_fracs nan", lambda: mix.check_fracs([0, 0.5, np.nan], 3), V, "dusp-hip: the fraction of voice 2 is not finite"),
    ("check_fracs one", lambda: mix.check_fracs([0, 1, 0.5], 3), V, "dusp-hip: the fraction of voice 1 is outside [0, 1)"),
    ("check_fracs negative", lambda: mix.check_fracs([-0.5, 0, 0.5], 3), V, "dusp-hip: the fraction of voice 0 is outside [0, 1)"),
    ("check_fracs finite+range", lambda: mix.check_fracs([7, 0, np.inf], 3), V, "dusp-hip: the fraction of voice 2 is not finite"),
    ("split_onsets nan", lambda: mix.split_onsets([0.5, np.nan]), V, "dusp-hip: positions are finite numbers of samples within int64"),
    ("split_onsets 2^63", lambda: mix.split_onsets([2.0 ** 63]), V, "dusp-hip: positions are finite numbers of samples within int64"),
    ("split_onsets below -2^63", lambda: mix.split_onsets([-2.0 ** 63 - 2048]), V, "dusp-hip: positions are finite numbers of samples within int64"),
    # ---- runtime: the argument helpers that need no device
    ("pan_arrays shape", lambda: runtime.pan_arrays([0, 0], 3), V, "dusp-hip: pans must have shape (voices=3,)"),
    ("pan_arrays nan", lambda: runtime.pan_arrays([0, 0.5, np.nan], 3), V, "dusp-hip: the pan of voice 2 is not finite"),
    ("pan_arrays beyond f32", lambda: runtime.pan_arrays([0, 1e39, np.nan], 3), V, "dusp-hip: the pan of voice 1 is not finite"),
    ("pan_arrays comp", lambda: runtime.pan_arrays([0, 0, 0], 3, comp=[1.0, 1.0]), V, "dusp-hip: comp must have shape (voices=3,)"),
    ("pan_arrays finite+comp", lambda: runtime.pan_arrays([np.inf, 0, 0], 3, comp=[1.0]), V, "dusp-hip: the pan of voice 0 is not finite"),
    ("frac_arrays shape", lambda: runtime.frac_arrays([[0, 0, 0]], 3), V, "dusp-hip: fracs must have shape (voices=3,)"),
    ("frac_arrays inf", lambda: runtime.frac_arrays([0, -np.inf, 0], 3), V, "dusp-hip: the fraction of voice 1 is not finite"),
    ("frac_arrays range", lambda: runtime.frac_arrays([0, 0, 1.5], 3), V, "dusp-hip: the fraction of voice 2 is outside [0, 1)"),
    ("frac_arrays shape+range", lambda: runtime.frac_arrays([7, 7], 3), V, "dusp-hip: fracs must have shape (voices=3,)"),
    ("_pcm_format", lambda: runtime._pcm_format("s8"), V, 'dusp-hip: format must be "s16", "s24" or "f32", not \'s8\''),
    ("_whole_samples shape", lambda: runtime._whole_samples([0, 1], 3, "onsets"), V, "dusp-hip: onsets must have shape (n_instances=3,)"),
    ("_whole_samples fraction", lambda: runtime._whole_samples([0, 1, 2.5], 3, "lengths"), V, IN_SAMPLES % "lengths"),
    ("_whole_samples nan", lambda: runtime._whole_samples([0, np.nan, 2], 3, "onsets"), V, IN_SAMPLES % "onsets"),
    ("_whole_samples 2^63", lambda: runtime._whole_samples([0, -2.0 ** 63, 2], 3, "onsets"), V, IN_SAMPLES % "onsets"),
    ("_whole_samples no number", lambda: runtime._whole_samples([True, False, True], 3, "onsets"), V, IN_SAMPLES % "onsets"),
    ("_whole_samples shape+fraction", lambda: runtime._whole_samples([0.5], 3, "onsets"), V, "dusp-hip: onsets must have shape (n_instances=3,)"),
    ("_score_rows row_samples shape", lambda: runtime._score_rows([1, 2], [24], [0, 1], None), V, "dusp-hip: row_samples must be whole numbers 0 .. 2^32 - 1 of shape (voices=2,)"),
    ("_score_rows row_samples real", lambda: runtime._score_rows([1, 2], [24.0, 17.0], [0, 1], None), V, "dusp-hip: row_samples must be whole numbers 0 .. 2^32 - 1 of shape (voices=2,)"),
    ("_score_rows row_samples negative", lambda: runtime._score_rows([1, 2], [24, -1], [0, 1], None), V, "dusp-hip: row_samples must be whole numbers 0 .. 2^32 - 1 of shape (voices=2,)"),
    ("_score_rows row_samples 2^32", lambda: runtime._score_rows([1, 2], [24, 2 ** 32], [0, 1], None), V, "dusp-hip: row_samples must be whole numbers 0 .. 2^32 - 1 of shape (voices=2,)"),
    ("_score_rows onsets", lambda: runtime._score_rows([1, 2], [24, 17], [0], None), V, "dusp-hip: onsets must have shape (n_instances=2,)"),
    ("_score_rows lengths", lambda: runtime._score_rows([1, None], [24, 0], [0, 1], [24, 0.5]), V, IN_SAMPLES % "lengths"),
    ("_score_rows row_samples+onsets", lambda: runtime._score_rows([1, 2], [24], [0.5, 1], None), V, "dusp-hip: row_samples must be whole numbers 0 .. 2^32 - 1 of shape (voices=2,)"),
    ("_score_rows onsets+lengths", lambda: runtime._score_rows([1, 2], [24, 17], [0, 0.5], [1]), V, IN_SAMPLES % "onsets"),
    # ---- render: what is refused before a context is made
    ("render_mix_pcm bit depth", lambda: d.render_mix_pcm(mono(), SHORT, bit_depth=8), W, BIT_DEPTH),
    ("render_mix_pcm normalise", lambda: d.render_mix_pcm(mono(), SHORT, normalise=3), W, NORMALISE),
    ("render_mix_pcm bit depth+normalise", lambda: d.render_mix_pcm(mono(), SHORT, 20, -1), W, BIT_DEPTH),
    ("render_mix_wav bit depth", lambda: d.render_mix_wav(mono(), SHORT, bit_depth=12), W, BIT_DEPTH),
    ("render_score no samples", lambda: d.render_score(mono(), [0, 1, 2], 0, SHORT), W, NO_SAMPLES),
    ("render_score negative duration", lambda: d.render_score(mono(), [0, 1, 2], SHORT, -1), W, "negative duration"),
    ("render_score onsets shape", lambda: d.render_score(mono(), [0, 1], SHORT, LONG), V, "dusp-hip: onsets must have shape (n_instances=3,)"),
    ("render_score onsets fraction", lambda: d.render_score(mono(), [0, 0.5, 2], SHORT, LONG), V, IN_SAMPLES % "onsets"),
    ("render_score lengths shape", lambda: d.render_score(mono(), [0, 1, 2], SHORT, LONG, lengths=[48]), V, "dusp-hip: lengths must have shape (n_instances=3,)"),
    ("render_score lengths fraction", lambda: d.render_score(mono(), [0, 1, 2], SHORT, LONG, lengths=[48, 47.5, 0]), V, IN_SAMPLES % "lengths"),
    ("render_score lengths long", lambda: d.render_score(mono(), [0, 1, 2], SHORT, LONG, lengths=[48, 49, 0]), V, "dusp-hip: lengths must lie in 0 .. the voice's 48 samples"),
    ("render_score lengths negative", lambda: d.render_score(mono(), [0, 1, 2], SHORT, LONG, lengths=[48, -1, 0]), V, "dusp-hip: lengths must lie in 0 .. the voice's 48 samples"),
    ("render_score gains", lambda: d.render_score(mono(), [0, 1, 2], SHORT, LONG, gains=[1, 1]), V, "dusp-hip: gains must have shape (n_instances=3,)"),
    ("render_score no samples+onsets", lambda: d.render_score(mono(), [0.5], 0, LONG), W, NO_SAMPLES),
    ("render_score onsets+lengths", lambda: d.render_score(mono(), [0, 1], SHORT, LONG, lengths=[99, 99, 99]), V, "dusp-hip: onsets must have shape (n_instances=3,)"),
    ("render_score lengths+gains", lambda: d.render_score(mono(), [0, 1, 2], SHORT, 0, lengths=[99, 99, 99], gains=[1]), V, "dusp-hip: lengths must lie in 0 .. the voice's 48 samples"),
    ("render_score pans, durations", lambda: d.render_score(mono(), [0, 1, 2], [SHORT] * 3, LONG, pans=[0, 0, 0]), V, ONE_NUMBER),
    ("render_score fracs, durations", lambda: d.render_score(mono(), [0, 1, 2], [SHORT] * 3, LONG, fracs=[0, 0, 0]), V, ONE_NUMBER),
    ("render_score pans shape", lambda: d.render_score(mono(), [0, 1, 2], SHORT, LONG, pans=[0, 0]), V, "dusp-hip: pans must have shape (voices=3,)"),
    ("render_score pans, gains", lambda: d.render_score(mono(), [0, 1, 2], SHORT, LONG, gains=[1], pans=[0, 0, 0]), V, "dusp-hip: gains must have shape (voices=3,)"),
    ("render_score pans, onsets", lambda: d.render_score(mono(), [0, 1], SHORT, LONG, pans=[0, 0, 0]), V, "dusp-hip: onsets must have shape (n_instances=3,)"),
    ("render_score pans, one part", lambda: d.render_score(two_structures(), [0, 1, 2], SHORT, LONG, pans=[0, 0, 0]), W, ONE_PART),
    ("render_score fracs, one part", lambda: d.render_score(two_structures(), [0, 1, 2], SHORT, 0, fracs=[0, 0, 0]), W, ONE_PART),
    ("render_score fracs range", lambda: d.render_score(mono(), [0, 1, 2], SHORT, LONG, fracs=[0, 1, 0]), V, "dusp-hip: the fraction of voice 1 is outside [0, 1)"),
    ("render_score pans+fracs", lambda: d.render_score(mono(), [0, 1, 2], SHORT, LONG, pans=[0, np.nan, 0], fracs=[0, 1, 0]), V, "dusp-hip: the pan of voice 1 is not finite"),
    ("render_score_pcm bit depth", lambda: d.render_score_pcm(mono(), [0, 1, 2], SHORT, LONG, bit_depth=0), W, BIT_DEPTH),
    ("render_score_pcm normalise", lambda: d.render_score_pcm(mono(), [0, 1, 2], SHORT, LONG, normalise=0.5), W, NORMALISE),
    ("render_score_pcm bit depth+no samples", lambda: d.render_score_pcm(mono(), [0, 1, 2], 0, LONG, bit_depth=8), W, BIT_DEPTH),
    ("render_score_pcm normalise+onsets", lambda: d.render_score_pcm(mono(), [0, 1], SHORT, LONG, normalise=3), W, NORMALISE),
    ("render_score_pcm no samples", lambda: d.render_score_pcm(mono(), [0, 1, 2], 0, LONG), W, NO_SAMPLES),
    ("render_score_pcm lengths", lambda: d.render_score_pcm(mono(), [0, 1, 2], SHORT, 0, lengths=[49, 0, 0]), V, "dusp-hip: lengths must lie in 0 .. the voice's 48 samples"),
    ("render_score_pcm gains", lambda: d.render_score_pcm(mono(), [0, 1, 2], SHORT, LONG, 24, 2, None, [1, 2]), V, "dusp-hip: gains must have shape (n_instances=3,)"),
    ("render_score_pcm pans, durations+bit depth", lambda: d.render_score_pcm(mono(), [0, 1, 2], [SHORT] * 3, LONG, bit_depth=8, pans=[0, 0, 0]), V, ONE_NUMBER),
    ("render_score_pcm pans, bit depth+pans", lambda: d.render_score_pcm(mono(), [0, 1, 2], SHORT, LONG, bit_depth=8, pans=[0, 0]), W, BIT_DEPTH),
    ("render_score_pcm fracs, normalise", lambda: d.render_score_pcm(mono(), [0, 1, 2], SHORT, LONG, normalise=7, fracs=[0, 0, 0]), W, NORMALISE),
    ("render_score_pcm fracs nan", lambda: d.render_score_pcm(mono(), [0, 1, 2], SHORT, LONG, fracs=[0, 0, np.nan]), V, "dusp-hip: the fraction of voice 2 is not finite"),
    ("render_score_pcm pans, one part", lambda: d.render_score_pcm(two_structures(), [0, 1, 2], SHORT, LONG, pans=[0, 0, 0]), W, ONE_PART),
    ("render_score_wav bit depth", lambda: d.render_score_wav(mono(), [0, 1, 2], SHORT, LONG, bit_depth=8), W, BIT_DEPTH),
    ("render_piece no voices", lambda: d.render_piece([], [], SHORT, LONG), W, "dusp-hip: no instances"),
    ("render_piece durations shape", lambda: d.render_piece(mono(), [0, 1, 2], [SHORT, LONG], LONG), V, "dusp-hip: voice_durations must be one number or have shape (voices=3,)"),
    ("render_piece no samples", lambda: d.render_piece(mono(), [0, 1, 2], [SHORT, 0, LONG], LONG), W, NO_SAMPLES),
    ("render_piece negative voice duration", lambda: d.render_piece(mono(), [0, 1, 2], [SHORT, -1, LONG], LONG), W, "negative duration"),
    ("render_piece onsets shape", lambda: d.render_piece(mono(), [0, 1, 2, 3], SHORT, LONG), V, "dusp-hip: onsets must have shape (n_instances=3,)"),
    ("render_piece onsets fraction", lambda: d.render_piece(mono(), [0, 0.5, 2], SHORT, LONG), V, IN_SAMPLES % "onsets"),
    ("render_piece lengths shape", lambda: d.render_piece(mono(), [0, 1, 2], SHORT, LONG, lengths=[1]), V, "dusp-hip: lengths must have shape (n_instances=3,)"),
    ("render_piece lengths long", lambda: d.render_piece(mono(), [0, 1, 2], [SHORT, LONG, SHORT], LONG, lengths=[48, 96, 49]), V, "dusp-hip: lengths must lie in 0 .. the voice's own samples"),
    ("render_piece lengths negative", lambda: d.render_piece(mono(), [0, 1, 2], SHORT, LONG, lengths=[-1, 0, 0]), V, "dusp-hip: lengths must lie in 0 .. the voice's own samples"),
    ("render_piece gains", lambda: d.render_piece(mono(), [0, 1, 2], SHORT, LONG, gains=[[1, 1, 1]]), V, "dusp-hip: gains must have shape (voices=3,)"),
    ("render_piece pans shape", lambda: d.render_piece(mono(), [0, 1, 2], SHORT, LONG, pans=[0, 0]), V, "dusp-hip: pans must have shape (voices=3,)"),
    ("render_piece pans inf", lambda: d.render_piece(mono(), [0, 1, 2], SHORT, LONG, pans=[0, 0, -np.inf]), V, "dusp-hip: the pan of voice 2 is not finite"),
    ("render_piece fracs shape", lambda: d.render_piece(mono(), [0, 1, 2], SHORT, LONG, fracs=[0, 0]), V, "dusp-hip: fracs must have shape (voices=3,)"),
    ("render_piece fracs nan", lambda: d.render_piece(mono(), [0, 1, 2], SHORT, LONG, fracs=[0, 0.5, np.nan]), V, "dusp-hip: the fraction of voice 2 is not finite"),
    ("render_piece fracs range", lambda: d.render_piece(mono(), [0, 1, 2], SHORT, LONG, fracs=[0, 1, 0.5]), V, "dusp-hip: the fraction of voice 1 is outside [0, 1)"),
    ("render_piece one part", lambda: d.render_piece(two_structures(), [0, 1, 2], SHORT, LONG, _one_part=True), W, ONE_PART),
    ("render_piece one part, by length", lambda: d.render_piece(mono(), [0, 1, 2], [SHORT, LONG, SHORT], LONG, _one_part=True), W, ONE_PART),
    ("render_piece channels", lambda: d.render_piece(two_channel_counts(), [0, 1, 2], SHORT, LONG), W, CHANNELS),
    ("render_piece channels, no timeline", lambda: d.render_piece(two_channel_counts(), [0, 1, 2], SHORT, 0), W, CHANNELS),
    ("render_piece panned channels", lambda: d.render_piece(two_channel_counts(), [0, 1, 2], SHORT, LONG, pans=[0, 0, 0]), W, NOT_MONO),
    ("render_piece durations+onsets", lambda: d.render_piece(mono(), [0], [SHORT], LONG), V, "dusp-hip: voice_durations must be one number or have shape (voices=3,)"),
    ("render_piece no samples+onsets", lambda: d.render_piece(mono(), [0], 0, LONG), W, NO_SAMPLES),
    ("render_piece onsets+lengths", lambda: d.render_piece(mono(), [0, 1, 2.5], SHORT, LONG, lengths=[99, 99, 99]), V, IN_SAMPLES % "onsets"),
    ("render_piece lengths+gains", lambda: d.render_piece(mono(), [0, 1, 2], SHORT, LONG, lengths=[49, 0, 0], gains=[1]), V, "dusp-hip: lengths must lie in 0 .. the voice's own samples"),
    ("render_piece gains+pans", lambda: d.render_piece(mono(), [0, 1, 2], SHORT, LONG, gains=[1], pans=[0]), V, "dusp-hip: gains must have shape (voices=3,)"),
    ("render_piece pans+fracs", lambda: d.render_piece(mono(), [0, 1, 2], SHORT, LONG, pans=[0], fracs=[0]), V, "dusp-hip: pans must have shape (voices=3,)"),
    ("render_piece fracs+channels", lambda: d.render_piece(two_channel_counts(), [0, 1, 2], SHORT, LONG, fracs=[0, 0, 2]), V, "dusp-hip: the fraction of voice 2 is outside [0, 1)"),
    ("render_piece one part+channels", lambda: d.render_piece(two_channel_counts(), [0, 1, 2], SHORT, LONG, _one_part=True), W, ONE_PART),
    ("render_piece_pcm bit depth", lambda: d.render_piece_pcm(mono(), [0, 1, 2], SHORT, LONG, bit_depth=8), W, BIT_DEPTH),
    ("render_piece_pcm normalise", lambda: d.render_piece_pcm(mono(), [0, 1, 2], SHORT, LONG, normalise=3), W, NORMALISE),
    ("render_piece_pcm bit depth+normalise", lambda: d.render_piece_pcm(mono(), [0, 1, 2], SHORT, LONG, 8, 3), W, BIT_DEPTH),
    ("render_piece_pcm normalise+no voices", lambda: d.render_piece_pcm([], [], SHORT, LONG, normalise=3), W, NORMALISE),
    ("render_piece_pcm no voices", lambda: d.render_piece_pcm([], [], SHORT, LONG), W, "dusp-hip: no instances"),
    ("render_piece_pcm durations shape", lambda: d.render_piece_pcm(mono(), [0, 1, 2], [[SHORT]], LONG), V, "dusp-hip: voice_durations must be one number or have shape (voices=3,)"),
    ("render_piece_pcm no samples", lambda: d.render_piece_pcm(mono(), [0, 1, 2], 1e-6, LONG), W, NO_SAMPLES),
    ("render_piece_pcm lengths", lambda: d.render_piece_pcm(mono(), [0, 1, 2], SHORT, 0, lengths=[0, 0, 49]), V, "dusp-hip: lengths must lie in 0 .. the voice's own samples"),
    ("render_piece_pcm gains", lambda: d.render_piece_pcm(mono(), [0, 1, 2], SHORT, LONG, gains=[1, 2]), V, "dusp-hip: gains must have shape (voices=3,)"),
    ("render_piece_pcm pans", lambda: d.render_piece_pcm(mono(), [0, 1, 2], SHORT, LONG, pans=[0, np.nan, np.nan]), V, "dusp-hip: the pan of voice 1 is not finite"),
    ("render_piece_pcm fracs", lambda: d.render_piece_pcm(mono(), [0, 1, 2], SHORT, LONG, fracs=[0, -0.5, 0.5]), V, "dusp-hip: the fraction of voice 1 is outside [0, 1)"),
    ("render_piece_pcm channels", lambda: d.render_piece_pcm(two_channel_counts(), [0, 1, 2], SHORT, LONG), W, CHANNELS),
    ("render_piece_pcm panned channels", lambda: d.render_piece_pcm(two_channel_counts(), [0, 1, 2], [SHORT, LONG, SHORT], 0, pans=[0, 0, 0]), W, NOT_MONO),
    ("render_piece_wav bit depth", lambda: d.render_piece_wav(mono(), [0, 1, 2], SHORT, LONG, bit_depth=8), W, BIT_DEPTH),
    ("render_piece_wav panned channels", lambda: d.render_piece_wav(two_channel_counts(), [0, 1, 2], SHORT, 0, pans=[0, 0, 0]), W, NOT_MONO),
    ("check_piece_channels", lambda: render.check_piece_channels([2, 2, 1]), W, "dusp-hip: the voices of a piece must have one number of output channels: part 2 has 1, part 0 has 2"),
    ("check_pan_channels", lambda: render.check_pan_channels([1, 2, 1]), W, NOT_MONO),
    ("check_pan_channels first of two", lambda: render.check_pan_channels([3, 2]), W, "dusp-hip: a panned voice is mono: part 0 has 3 output channels"),
]

TYPES = {V: ValueError, W: DuspError}


def refusal(call):
    """-> (name of the exception's own type, its message)"""
    d.configure(sv.SAMPLE_RATE)
    with pytest.raises(Exception) as e:
        call()
    return type(e.value).__name__, str(e.value)


def test_the_table_names_every_case_once():
    names = [name for name, _, _, _ in CASES]
    assert len(set(names)) == len(names)
    for family in ("mix_chain", "score_chain", "rows", "panned", "_score_rows", "render_score", "render_score_pcm", "render_piece", "render_piece_pcm"):
        assert any(name.startswith(family + " ") and "+" in name for name in names), "no case of two bad arguments for " + family


@pytest.mark.parametrize("name,call,exception,message", CASES, ids=[c[0] for c in CASES])
def test_the_refusal_is_todays_by_type_and_full_message(name, call, exception, message):
    got_type, got_message = refusal(call)
    assert (got_type, got_message) == (TYPES[exception].__name__, message)


def test_what_is_well_formed_is_not_refused():
    """the neighbours of the refusals above: the table's calls fail for the reason named, not for the way the table builds its arguments"""
    assert mix.mix_chain(P, gains=[1, 2], init=np.zeros((1, 24))).shape == (1, 24)
    assert mix.score_chain(P, [0.0, -3], 30.0, lengths=[24, 0], gains=[1, 2], init=np.zeros((1, 30))).shape == (1, 30)
    assert mix.score_chain_rows([A, B], [0, 1], 30, lengths=[24, 17], gains=[1, 2], fracs=[0, 0.5], init=np.zeros((1, 30))).shape == (1, 30)
    assert mix.score_chain_rows([], [], 30, init=np.zeros((3, 30))).shape == (3, 30)
    assert mix.score_chain_rows_panned([A, B], [0, 1], [0, 1.5], 30, lengths=[24, 17], gains=[1, 2], comp=[1, 1], fracs=[0, 0.5], init=np.zeros((2, 30))).shape == (2, 30)
    assert runtime._whole_samples([0.0, -1.0, 2], 3, "onsets").dtype == np.int64
    pointers, samples, onsets, lengths = runtime._score_rows([1, None], [24, 0], [0, 1], [24, 0])
    assert pointers.tolist() == [1, 0] and samples.dtype == np.uint32 and onsets.dtype == lengths.dtype == np.int64
    assert runtime._score_rows([], [], [], None)[1].shape == (0,)
    assert len(d.render_piece(mono(), [0, 1, 2], [SHORT, LONG, SHORT], 0, lengths=[48, 96, 48], gains=[1, 1, 1], pans=[0, 0, 0], fracs=[0, 0.5, 0])) == 0
