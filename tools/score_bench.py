#!/usr/bin/env python3
"""Score rendering, measured (run by hand on the GPU; the output is kept as profiles/score_mix.txt).

  dense   the score kernel with every onset 0 and full lengths — the mix, as a score — over rows of the shapes of mix_bench.py's cases
          a-d (seeded noise: the kernels' time does not depend on the values), against dusp_mix_device over the same rows, which is the
          yardstick, and against bytes read / the float4-copy rate.  The mix kernel by HIP events on the launch stream (its call does no
          host work); the score kernel by the events the library records around the launch alone (dusp_score_last_ms), with the plan's
          host time and the upload's time, which precede the launch inside the call, reported beside it.  The plan's default block and a
          block forced to cover the whole timeline (DUSP_SCORE_PLAN_KB=1: one list for every workgroup) side by side.  Then the rows
          kernel (dusp_score_rows_device) over the same buffer, its rows handed over as pointers of their own (profiles/score_rows.txt).
  pan     (--pan; profiles/score_pan.txt) the panned kernel (dusp_score_rows_pan_device) over dense MONO rows of the dense shapes, kernel
          alone by dusp_score_last_ms, against dusp_score_rows_device over the same voices as TWO-CHANNEL rows — unchanged code, and what a
          panned piece costs without it: every voice a two-channel circuit with a Pan unit inside.
  frac    (--frac; profiles/score_frac.txt) the two-tap kernel (dusp_score_rows_frac_device) over dense MONO rows of the dense shapes, every
          fraction non-zero — plain, with gains and panned — kernel alone by dusp_score_last_ms, against dusp_score_rows_device (and
          dusp_score_rows_pan_device for the panned case) over the same rows, which is unchanged code; and the new entry point with all
          fractions zero, which launches those kernels.
  space   (--space; profiles/score_space.txt) the space kernel (dusp_score_rows_space_device) over dense MONO rows of the dense shapes,
          kernel alone by dusp_score_last_ms: two speakers with every delay fractional, against the panned two-tap kernel over the same
          rows with every fraction non-zero (the same four taps per output pair; unchanged code) and against the whole-sample panned
          kernel; two speakers with every delay whole; six speakers with every delay fractional.
  stereo  (--stereo; profiles/score_stereo.txt) the stereo kernel (dusp_score_rows_stereo_device) over dense rows of the dense shapes,
          kernel alone by dusp_score_last_ms: all voices mono and panned, against the panned kernel over the same rows; all voices of two
          channels, against the rows kernel over the same rows (both unchanged code); and a list that cycles through panned mono, plain
          mono and two channels.  A report: no ratio is fixed in advance.
  piece   8192 notes of 0.5 s placed over 60 s in onset order: Program.render_score on the host's clock, against the render of the same
          notes alone (render_device into a preallocated buffer) and against the same piece with the onsets shuffled — every tile's
          union window is then the whole timeline, which is what the window is worth.  One run under DUSP_JIT_LOG=2 prints the plans'
          host time and block (stderr).
  master  (--master; profiles/score_master.txt) the piece above — 8192 notes of 0.5 s over 60 s in onset order — through
          Context.render_score_parts without a master and with a Clip master, an echo master and a Filter master
          (dusp_render_host_score_piece): the call on the host's clock, and the master's render alone
          (dusp_last_kernel_ms on the master program).  A report: no ratio is fixed in advance.
  sends   (--sends; profiles/score_sends.txt) the same piece's notes, rendered once into device rows, one channel and panned: the
          send kernel (dusp_score_rows_send_device) at 1, 2 and 4 buses against the rows (resp. pan) kernel with
          gains over the same plan — launched once, the floor: what the dry chain alone costs; and 1 + B times into distinct
          buffers, what reading every row once is meant to beat.  The return kernel against dusp_fill_device.  The whole call on
          the host's clock with an echo bus and without.  A report: no ratio is fixed in advance.
  tracks  (--tracks; profiles/score_tracks.txt) the mix kernel (dusp_score_tracks_mix_device) over one channel of
          the piece's timeline at T = 2, 4, 8 tracks and B = 0, 2 buses, with faders, against dusp_fill_device over one timeline
          and against the return kernel over as many input buffers (T <= 4).  Then the piece with eight Filter tracks as ONE
          program of eight instances on the host's clock, beside the piece with the same Filter as its master, the piece
          alone, and eight calls with the Filter as the master one after the other.  A report: no ratio is fixed in advance.
  stems   (--stems; profiles/score_stems.txt) the stems mix kernel (dusp_score_stems_mix_device) over one channel of
          the piece's timeline at T = 8 tracks with faders and B = 2 buses against the mix kernel of the tracks over the same inputs,
          and the stems return kernel against the return kernel.  Then the piece with eight fader groups and two stateless buses
          on the host's clock: with stems, without, and the eleven single-stem calls (all faders but one 0) the call with stems
          replaces, one after the other.  A report: no ratio is fixed in advance.
  meters  (--meters; profiles/score_meters.txt) the meter kernels (dusp_meter_device) over the twelve signals of the
          stems' case, one channel and two, pass by pass by HIP events (dusp_meter_last_ms), beside dusp_pcm_peak_kernel over the same
          block; then the piece with stems on the host's clock with and without meters=True, one channel and panned into two.  With
          DUSP_HIP_LIB naming a library from before the meters the call with stems alone.  A report: no ratio is fixed in advance.
  loudness (--loudness; profiles/score_loudness.txt) the true-peak kernel (dusp_true_peak_device) over the same twelve
          signals, beside the peak kernel and the meter passes; then the piece with stems as s16 frames with meters=True,
          normalise=2, with true_peak=True and with loudness=-16, and without any new option — the only leg under DUSP_HIP_LIB
          naming the parent's library.  A report: no ratio is fixed in advance.
  limiter release (--limiter-release; profiles/score_limiter_release.txt) the launches of a limiter call with a release of its own, by HIP
          events, beside dusp_limit_apply_kernel; the piece with stems at a loudness target with and without limiter_release
  limiter (--limiter; profiles/score_limiter.txt) the limiter's two kernels (dusp_limit_device, kernel by kernel by HIP events:
          dusp_limit_last_ms) over the same twelve signals with a window of 240 samples: the envelope kernel beside
          the true-peak kernel, the gain / apply kernel beside the peak kernel; then the piece with stems as s16 frames at a
          loudness target with the limiter engaged, with the limiter not engaged, and without it — the only leg under DUSP_HIP_LIB
          naming the parent's library.  A report: no ratio is fixed in advance.

Every variant is timed `--reps` times after a warm-up call; lines give the median and the fastest.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dusp_amd as d  # noqa: E402
from dusp_amd import descriptor  # noqa: E402
from mix_bench import COPY_RATE, SR, context, timed  # noqa: E402

DENSE = {"a": (8192, 10 * SR), "b": (1024, 60 * SR), "c": (16384, SR), "d": (65536, SR)}  # voices, samples (one channel)


def dense(key, scale, ctxs, reps):
    import torch
    V, n = max(64, DENSE[key][0] // scale), DENSE[key][1]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rows = torch.empty((V, 1, n), dtype=torch.float32, device="cuda").normal_()
    acc = torch.empty((1, n), dtype=torch.float32, device="cuda")
    onsets = np.zeros(V, dtype=np.int64)
    torch.cuda.synchronize()
    read = (V + 0) * n * 4
    print("dense %s: %d rows x %d samples = %.2f GB of f32; bytes / %.2f TB/s = %.3f ms" % (key, V, n, read / 1e9, COPY_RATE / 1e12, read / COPY_RATE * 1e3), flush=True)
    med, best = timed(lambda: ctxs["default"].mix(rows.data_ptr(), V, 1, n, acc.data_ptr(), None, None, False, s), stream, reps)
    t_mix = med
    line = "  %-30s kernel median %9.3f ms  fastest %9.3f   %6.2f TB/s = %4.1f%% of the copy rate   x%.3f of the mix kernel by grid%s"
    rate = lambda ms: (read / ms / 1e9, 100 * read / ms * 1e3 / COPY_RATE, ms / t_mix)
    print(line % (("mix kernel, by grid", med, best) + rate(med) + ("",)), flush=True)
    med, best = timed(lambda: ctxs["dword8"].mix(rows.data_ptr(), V, 1, n, acc.data_ptr(), None, None, False, s), stream, reps)
    print(line % (("mix kernel, 1 float x 8", med, best) + rate(med) + ("",)), flush=True)
    # the score kernel ALONE: events around the launch inside the library (dusp_score_last_ms), behind the plan and its upload, which
    # are host work and a copy of their own and are reported beside it
    for label, ctx in [("score kernel, default block", ctxs["default"]), ("score kernel, one block", ctxs["one_block"])]:
        kernel, plan, upload = [], [], []
        for r in range(reps + 1):
            ctx.score_device(rows.data_ptr(), V, 1, n, onsets, n, acc.data_ptr(), stream=s)
            k, p, u = ctx.score_last_ms()
            if r:
                kernel.append(k), plan.append(p), upload.append(u)
        med = float(np.median(kernel))
        print(line % ((label, med, min(kernel)) + rate(med) + ("   [plan on the host %.2f ms, its upload %.2f ms]" % (float(np.median(plan)), float(np.median(upload))),)), flush=True)
    # the rows kernel (dusp_score_rows_device) over the SAME buffer, every row handed over as a pointer of its own: what the 32-byte record
    # and the address taken from it cost against the score kernel above, which is the yardstick (profiles/score_rows.txt)
    pointers = [rows.data_ptr() + 4 * n * k for k in range(V)]
    samples = np.full(V, n, dtype=np.uint32)
    kernel, plan, upload = [], [], []
    for r in range(reps + 1):
        ctxs["default"].score_rows_device(pointers, samples, 1, onsets, n, acc.data_ptr(), stream=s)
        k, p, u = ctxs["default"].score_last_ms()
        if r:
            kernel.append(k), plan.append(p), upload.append(u)
    med = float(np.median(kernel))
    print(line % (("rows kernel, default block", med, min(kernel)) + rate(med) + ("   [plan on the host %.2f ms, its upload %.2f ms]" % (float(np.median(plan)), float(np.median(upload))),)), flush=True)


def pan(key, scale, ctxs, reps):
    import torch
    V, n = max(64, DENSE[key][0] // scale), DENSE[key][1]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = ctxs["default"]
    onsets = np.zeros(V, dtype=np.int64)
    samples = np.full(V, n, dtype=np.uint32)
    pans = (np.random.RandomState(5).random_sample(V) * 2 - 1).astype(np.float32)
    acc = torch.empty((2, n), dtype=torch.float32, device="cuda")

    def median_of(call):
        kernel, plan, upload = [], [], []
        for r in range(reps + 1):
            call()
            k, p, u = ctx.score_last_ms()
            if r:
                kernel.append(k), plan.append(p), upload.append(u)
        return float(np.median(kernel)), min(kernel), float(np.median(plan)), float(np.median(upload))

    line = "  %-44s kernel median %9.3f ms  fastest %9.3f   %6.2f GB read = %5.2f TB/s   [plan on the host %.2f ms, its upload %.2f ms]"
    print("pan %s: %d voices x %d samples, all onsets 0, full lengths, into a timeline of 2 x %d" % (key, V, n, n), flush=True)
    # the yardstick first, and its rows freed before the mono ones are made: (b) is 23.6 GB of two-channel rows
    wide = torch.empty((V, 2, n), dtype=torch.float32, device="cuda").normal_()
    torch.cuda.synchronize()
    pointers = [wide.data_ptr() + 8 * n * k for k in range(V)]
    t_wide = median_of(lambda: ctx.score_rows_device(pointers, samples, 2, onsets, n, acc.data_ptr(), stream=s))
    read = V * 2 * n * 4
    print(line % (("rows kernel over two-channel rows", t_wide[0], t_wide[1], read / 1e9, read / t_wide[0] / 1e9) + t_wide[2:]), flush=True)
    del wide
    mono = torch.empty((V, 1, n), dtype=torch.float32, device="cuda").normal_()
    torch.cuda.synchronize()
    pointers = [mono.data_ptr() + 4 * n * k for k in range(V)]
    t_pan = median_of(lambda: ctx.score_rows_pan(pointers, samples, onsets, pans, n, acc.data_ptr(), stream=s))
    read = V * n * 4
    print(line % (("panned kernel over mono rows", t_pan[0], t_pan[1], read / 1e9, read / t_pan[0] / 1e9) + t_pan[2:]), flush=True)
    d_gains = torch.ones(V, dtype=torch.float32, device="cuda")
    t_gain = median_of(lambda: ctx.score_rows_pan(pointers, samples, onsets, pans, n, acc.data_ptr(), d_gains=d_gains.data_ptr(), stream=s))
    print(line % (("panned kernel over mono rows, with gains", t_gain[0], t_gain[1], read / 1e9, read / t_gain[0] / 1e9) + t_gain[2:]), flush=True)
    print("  panned / two-channel rows: x%.3f (with gains x%.3f); %.1f voice terms per ns and channel pair" % (t_pan[0] / t_wide[0], t_gain[0] / t_wide[0], V * n / t_pan[0] / 1e6), flush=True)


def frac(key, scale, ctxs, reps):
    import torch
    V, n = max(64, DENSE[key][0] // scale), DENSE[key][1]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = ctxs["default"]
    onsets = np.zeros(V, dtype=np.int64)
    samples = np.full(V, n, dtype=np.uint32)
    rng = np.random.RandomState(6)
    pans = (rng.random_sample(V) * 2 - 1).astype(np.float32)
    fracs = rng.randint(1, 1024, V) / 1024.0
    zeros = np.zeros(V)
    mono = torch.empty((V, 1, n), dtype=torch.float32, device="cuda").normal_()
    acc = torch.empty((2, n), dtype=torch.float32, device="cuda")
    d_gains = torch.ones(V, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pointers = [mono.data_ptr() + 4 * n * k for k in range(V)]
    read = V * n * 4

    def median_of(call):
        kernel, plan, upload = [], [], []
        for r in range(reps + 1):
            call()
            k, p, u = ctx.score_last_ms()
            if r:
                kernel.append(k), plan.append(p), upload.append(u)
        return float(np.median(kernel)), min(kernel), float(np.median(plan)), float(np.median(upload))

    line = "  %-52s kernel median %9.3f ms  fastest %9.3f   %5.2f TB/s of rows   x%.3f   [plan on the host %.2f ms, its upload %.2f ms]"
    print("frac %s: %d mono voices x %d samples = %.2f GB of rows, all onsets 0, full lengths" % (key, V, n, read / 1e9), flush=True)
    g = d_gains.data_ptr()
    for label, old, new, zero in [
        ("plain", lambda: ctx.score_rows_device(pointers, samples, 1, onsets, n, acc.data_ptr(), stream=s),
         lambda: ctx.score_rows_frac(pointers, samples, 1, onsets, fracs, n, acc.data_ptr(), stream=s),
         lambda: ctx.score_rows_frac(pointers, samples, 1, onsets, zeros, n, acc.data_ptr(), stream=s)),
        ("gains", lambda: ctx.score_rows_device(pointers, samples, 1, onsets, n, acc.data_ptr(), d_gains=g, stream=s),
         lambda: ctx.score_rows_frac(pointers, samples, 1, onsets, fracs, n, acc.data_ptr(), d_gains=g, stream=s), None),
        ("panned", lambda: ctx.score_rows_pan(pointers, samples, onsets, pans, n, acc.data_ptr(), stream=s),
         lambda: ctx.score_rows_frac(pointers, samples, 1, onsets, fracs, n, acc.data_ptr(), pans=pans, stream=s),
         lambda: ctx.score_rows_frac(pointers, samples, 1, onsets, zeros, n, acc.data_ptr(), pans=pans, stream=s)),
        ("panned, gains", lambda: ctx.score_rows_pan(pointers, samples, onsets, pans, n, acc.data_ptr(), d_gains=g, stream=s),
         lambda: ctx.score_rows_frac(pointers, samples, 1, onsets, fracs, n, acc.data_ptr(), d_gains=g, pans=pans, stream=s), None),
    ]:
        t_old = median_of(old)
        print(line % (("%s: whole-sample kernel (unchanged code)" % label, t_old[0], t_old[1], read / t_old[0] / 1e9, 1.0) + t_old[2:]), flush=True)
        t_new = median_of(new)
        print(line % (("%s: two-tap kernel, every fraction non-zero" % label, t_new[0], t_new[1], read / t_new[0] / 1e9, t_new[0] / t_old[0]) + t_new[2:]), flush=True)
        if zero:
            t_zero = median_of(zero)
            print(line % (("%s: new entry point, all fractions zero" % label, t_zero[0], t_zero[1], read / t_zero[0] / 1e9, t_zero[0] / t_old[0]) + t_zero[2:]), flush=True)


def space(key, scale, ctxs, reps):
    import torch
    V, n = max(64, DENSE[key][0] // scale), DENSE[key][1]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = ctxs["default"]
    onsets = np.zeros(V, dtype=np.int64)
    samples = np.full(V, n, dtype=np.uint32)
    rng = np.random.RandomState(7)
    pans = (rng.random_sample(V) * 2 - 1).astype(np.float32)
    fracs = rng.randint(1, 1024, V) / 1024.0
    # delays up to 1024 samples (7 m at 48 kHz), every one with a fraction; gains as -3 dB a metre gives them
    delays = {C: rng.randint(0, 1024, (V, C)) + rng.randint(1, 1024, (V, C)) / 1024.0 for C in (2, 6)}
    tap_gains = {C: 10.0 ** (-3.0 * delays[C] / 140.0 / 20.0) for C in (2, 6)}
    mono = torch.empty((V, 1, n), dtype=torch.float32, device="cuda").normal_()
    acc = torch.empty((6, n), dtype=torch.float32, device="cuda")
    d_gains = torch.ones(V, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pointers = [mono.data_ptr() + 4 * n * k for k in range(V)]
    read = V * n * 4

    def median_of(call):
        kernel, plan, upload = [], [], []
        for r in range(reps + 1):
            call()
            k, p, u = ctx.score_last_ms()
            if r:
                kernel.append(k), plan.append(p), upload.append(u)
        return float(np.median(kernel)), min(kernel), float(np.median(plan)), float(np.median(upload))

    line = "  %-56s kernel median %9.3f ms  fastest %9.3f   %5.2f TB/s of rows   x%.3f   [plan on the host %.2f ms, its upload %.2f ms]"
    print("space %s: %d mono voices x %d samples = %.2f GB of rows, all onsets 0, full lengths" % (key, V, n, read / 1e9), flush=True)
    g = d_gains.data_ptr()
    t_pan = median_of(lambda: ctx.score_rows_pan(pointers, samples, onsets, pans, n, acc.data_ptr(), stream=s))
    print(line % (("panned whole-sample kernel (unchanged code)", t_pan[0], t_pan[1], read / t_pan[0] / 1e9, t_pan[0] / t_pan[0]) + t_pan[2:]), flush=True)
    t_two = median_of(lambda: ctx.score_rows_frac(pointers, samples, 1, onsets, fracs, n, acc.data_ptr(), pans=pans, stream=s))
    print(line % (("panned two-tap kernel, every fraction non-zero (unchanged)", t_two[0], t_two[1], read / t_two[0] / 1e9, t_two[0] / t_pan[0]) + t_two[2:]), flush=True)
    for label, C, dl, kw in [("space kernel, 2 speakers, every delay fractional", 2, delays[2], {}),
                             ("space kernel, 2 speakers, fractional, with gains", 2, delays[2], {"d_gains": g}),
                             ("space kernel, 2 speakers, every delay whole", 2, np.floor(delays[2]), {}),
                             ("space kernel, 6 speakers, every delay fractional", 6, delays[6], {})]:
        t = median_of(lambda: ctx.score_rows_space(pointers, samples, onsets, dl, tap_gains[C], n, acc.data_ptr(), stream=s, **kw))
        print(line % ((label, t[0], t[1], read / t[0] / 1e9, t[0] / t_pan[0]) + t[2:]) + "   x%.3f of the panned two-tap kernel" % (t[0] / t_two[0]), flush=True)


def stereo(key, scale, ctxs, reps):
    import torch
    V, n = max(64, DENSE[key][0] // scale), DENSE[key][1]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ctx = ctxs["default"]
    onsets = np.zeros(V, dtype=np.int64)
    samples = np.full(V, n, dtype=np.uint32)
    pans = (np.random.RandomState(5).random_sample(V) * 2 - 1).astype(np.float32)
    acc = torch.empty((2, n), dtype=torch.float32, device="cuda")

    def median_of(call):
        kernel, plan, upload = [], [], []
        for r in range(reps + 1):
            call()
            k, p, u = ctx.score_last_ms()
            if r:
                kernel.append(k), plan.append(p), upload.append(u)
        return float(np.median(kernel)), min(kernel), float(np.median(plan)), float(np.median(upload))

    line = "  %-44s kernel median %9.3f ms  fastest %9.3f   %6.2f GB read = %5.2f TB/s   [plan on the host %.2f ms, its upload %.2f ms]"
    show = lambda label, t, read: print(line % ((label, t[0], t[1], read / 1e9, read / t[0] / 1e9) + t[2:]), flush=True)
    print("stereo %s: %d voices x %d samples, all onsets 0, full lengths, into a timeline of 2 x %d" % (key, V, n, n), flush=True)
    # one buffer of two-channel rows; a mono voice's row is the first channel of its own
    wide = torch.empty((V, 2, n), dtype=torch.float32, device="cuda").normal_()
    torch.cuda.synchronize()
    pointers = [wide.data_ptr() + 8 * n * k for k in range(V)]
    ones, twos, unplaced = np.ones(V, dtype=np.uint32), np.full(V, 2, dtype=np.uint32), np.full(V, np.nan, dtype=np.float32)
    t_pan = median_of(lambda: ctx.score_rows_pan(pointers, samples, onsets, pans, n, acc.data_ptr(), stream=s))
    show("panned kernel over mono rows", t_pan, V * n * 4)
    t_all_pan = median_of(lambda: ctx.score_rows_stereo(pointers, samples, ones, onsets, pans, n, acc.data_ptr(), stream=s))
    show("stereo kernel, all voices mono and panned", t_all_pan, V * n * 4)
    t_rows = median_of(lambda: ctx.score_rows_device(pointers, samples, 2, onsets, n, acc.data_ptr(), stream=s))
    show("rows kernel over two-channel rows", t_rows, V * 2 * n * 4)
    t_all_two = median_of(lambda: ctx.score_rows_stereo(pointers, samples, twos, onsets, unplaced, n, acc.data_ptr(), stream=s))
    show("stereo kernel, all voices of two channels", t_all_two, V * 2 * n * 4)
    t_mono = median_of(lambda: ctx.score_rows_stereo(pointers, samples, ones, onsets, unplaced, n, acc.data_ptr(), stream=s))
    show("stereo kernel, all voices plain mono", t_mono, V * n * 4)
    kinds = np.arange(V) % 3  # panned mono, plain mono, two channels, ...
    channels = np.where(kinds == 2, 2, 1).astype(np.uint32)
    t_cycle = median_of(lambda: ctx.score_rows_stereo(pointers, samples, channels, onsets, np.where(kinds == 0, pans, np.float32(np.nan)).astype(np.float32), n, acc.data_ptr(), stream=s))
    show("stereo kernel, the three kinds in turn", t_cycle, int(channels.sum()) * n * 4)
    d_gains = torch.ones(V, dtype=torch.float32, device="cuda")
    t_gain = median_of(lambda: ctx.score_rows_stereo(pointers, samples, channels, onsets, np.where(kinds == 0, pans, np.float32(np.nan)).astype(np.float32), n, acc.data_ptr(),
                                                     d_gains=d_gains.data_ptr(), stream=s))
    show("stereo kernel, the three kinds, with gains", t_gain, int(channels.sum()) * n * 4)
    print("  stereo / panned kernel, all panned: x%.3f; stereo / rows kernel, all two-channel: x%.3f" % (t_all_pan[0] / t_pan[0], t_all_two[0] / t_rows[0]), flush=True)


def piece(scale, ctxs, reps):
    import torch
    V, nv, nt = max(64, 8192 // scale), SR // 2, 60 * SR
    d.configure(SR)
    note = lambda k: d.Multiply(d.Osc(110.0 + k / 8), d.Ramp(nv, 1, 0).trigger())
    uni = descriptor.unify([descriptor.extract(note(k)) for k in (0, 1)])
    params = (110.0 + np.arange(V, dtype=np.float64) / 8).astype(np.float32).reshape(1, V)
    in_order = np.sort(np.random.RandomState(1).randint(0, nt - nv, V)).astype(np.int64)
    shuffled = np.random.RandomState(2).permutation(in_order)
    prog = ctxs["default"].build(uni.words)
    stream = torch.cuda.Stream()
    out = torch.empty((V, prog.n_out_channels, nv), dtype=torch.float32, device="cuda")
    dp = torch.from_numpy(params).cuda()
    torch.cuda.synchronize()
    med, best = timed(lambda: prog.render_device(nv, V, dp.data_ptr(), out.data_ptr(), stream.cuda_stream), stream, reps)
    print("piece: %d notes of %d samples over %d samples (%.0f MB of notes, %.1f MB of timeline), engine %s" % (V, nv, nt, V * nv * 4 / 1e6, nt * 4 / 1e6, prog.engine), flush=True)
    print("  render of the notes alone (HIP events)         median %9.3f ms  fastest %9.3f   [%s]" % (med, best, prog.read_shape()), flush=True)
    del out
    for label, onsets, tile in [("onset order, default tile", in_order, 0), ("onset order, tiles of 1024", in_order, 1024), ("shuffled, default tile", shuffled, 0),
                                ("shuffled, tiles of 1024", shuffled, 1024)]:
        times = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            res = prog.render_score(nv, nt, V, onsets, None, params, tile_instances=tile, pinned=True)
            times.append((time.perf_counter() - t0) * 1e3)
            del res
        print("  render_score, host clock, %-27s median %9.2f ms  fastest %9.2f" % (label, float(np.median(times[1:])), min(times[1:])), flush=True)
    prog.close()
    logged = ctxs["log"].build(uni.words)
    print("  (DUSP_JIT_LOG=2, stderr: the plans' host time and block)", flush=True)
    logged.render_score(nv, nt, V, in_order, None, params, tile_instances=1024)
    logged.render_score(nv, nt, V, shuffled, None, params)
    logged.close()


def master(scale, ctxs, reps):
    V, nv, nt = max(64, 8192 // scale), SR // 2, 60 * SR
    d.configure(SR)
    note = lambda k: d.Multiply(d.Osc(110.0 + k / 8), d.Ramp(nv, 1, 0).trigger())
    uni = descriptor.unify([descriptor.extract(note(k)) for k in (0, 1)])
    params = (110.0 + np.arange(V, dtype=np.float64) / 8).astype(np.float32).reshape(1, V)
    onsets = np.sort(np.random.RandomState(1).randint(0, nt - nv, V)).astype(np.int64)
    ctx = ctxs["default"]
    prog = ctx.build(uni.words)

    def clip(x):
        c = d.Clip(0.8)
        c.IN = d.Multiply(x, 1.7)
        return c

    def echo(x):
        s = d.Sum(x, 0)
        s.B = d.Multiply(d.Delay(s, 300.25, 2048), 0.5)
        return s

    print("master: %d notes of %d samples over %d samples, one channel (%.1f MB of timeline, as much again for the master's output), engine %s" % (V, nv, nt, nt * 4 / 1e6, prog.engine),
          flush=True)
    for label, fx in [("no master", None), ("Clip(0.8) behind Multiply(x, 1.7)", clip), ("feedback echo, 300.25 samples", echo), ("Filter(x, 1200)", lambda x: d.Filter(x, 1200))]:
        through = ctx.build(descriptor.extract(fx(d.MasterInput())).words) if fx else None
        times, kernel = [], []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            res = ctx.render_score_parts([(prog, nv, V, params)], np.zeros(V, dtype=np.uint32), onsets, nt, pinned=True, master=(through, None) if through else None)
            times.append((time.perf_counter() - t0) * 1e3)
            del res
            if through:
                kernel.append(through.last_kernel_ms())
        shape = "   master render alone median %9.3f ms  fastest %9.3f   [%s]" % (float(np.median(kernel[1:])), min(kernel[1:]), through.read_shape()) if through else ""
        print("  render_score_parts, host clock, %-36s median %9.2f ms  fastest %9.2f%s" % (label, float(np.median(times[1:])), min(times[1:]), shape), flush=True)
        if through:
            through.close()
    prog.close()


def sends(scale, ctxs, reps):
    import torch
    V, nv, nt = max(64, 8192 // scale), SR // 2, 60 * SR
    d.configure(SR)
    note = lambda k: d.Multiply(d.Osc(110.0 + k / 8), d.Ramp(nv, 1, 0).trigger())
    uni = descriptor.unify([descriptor.extract(note(k)) for k in (0, 1)])
    params = (110.0 + np.arange(V, dtype=np.float64) / 8).astype(np.float32).reshape(1, V)
    onsets = np.sort(np.random.RandomState(1).randint(0, nt - nv, V)).astype(np.int64)
    ctx = ctxs["default"]
    prog = ctx.build(uni.words)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rows = torch.empty((V, 1, nv), dtype=torch.float32, device="cuda")
    dp = torch.from_numpy(params).cuda()
    prog.render_device(nv, V, dp.data_ptr(), rows.data_ptr(), s)
    torch.cuda.synchronize()
    pointers, samples = [rows.data_ptr() + 4 * nv * k for k in range(V)], np.full(V, nv, dtype=np.uint32)
    rs = np.random.RandomState(3)
    d_gains = torch.from_numpy((0.05 + 1.9 * rs.random_sample(V)).astype(np.float32)).cuda()
    pans = (rs.random_sample(V) * 2 - 1).astype(np.float32)
    levels = rs.random_sample((4, V)).astype(np.float32)

    def median_of(call, launches=1):
        kernel = []
        for r in range(reps + 1):
            total = 0.0
            for i in range(launches):
                call(i)
                total += ctx.score_last_ms()[0]
            if r:
                kernel.append(total)
        return float(np.median(kernel)), min(kernel)

    print("sends: %d notes of %d samples over %d samples (%.0f MB of notes, %.1f MB a timeline and channel), kernels alone by HIP events (dusp_score_last_ms), median and fastest of %d after a warm-up"
          % (V, nv, nt, V * nv * 4 / 1e6, nt * 4 / 1e6, reps), flush=True)
    line = "  %-58s median %8.3f ms  fastest %8.3f%s"
    for label, C, pan in (("rows, one channel", 1, None), ("panned, two channels", 2, pans)):
        bufs = [torch.zeros((C, nt), dtype=torch.float32, device="cuda") for _ in range(5)]
        snd = torch.zeros((4, C, nt), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        if pan is None:
            old = lambda i: ctx.score_rows_device(pointers, samples, 1, onsets, nt, bufs[i].data_ptr(), d_gains=d_gains.data_ptr(), raw=True, stream=s)
        else:
            old = lambda i: ctx.score_rows_pan(pointers, samples, onsets, pan, nt, bufs[i].data_ptr(), d_gains=d_gains.data_ptr(), raw=True, stream=s)
        floor = median_of(old)
        print(line % ((label + ": the kernel that stands, with gains, once (the floor)",) + floor + ("",)), flush=True)
        for B in (1, 2, 4):
            again = median_of(old, 1 + B)
            fused = median_of(lambda i: ctx.score_rows_send(pointers, samples, 1, onsets, levels[:B], nt, bufs[0].data_ptr(), snd.data_ptr(), d_gains=d_gains.data_ptr(), raw=True,
                                                            pans=pan, stream=s))
            print(line % ((label + ": the kernel that stands, %d launches into distinct buffers" % (1 + B),) + again + ("",)), flush=True)
            print(line % ((label + ": the send kernel, B = %d" % B,) + fused + ("   x%.2f of the floor, x%.2f of %d launches" % (fused[0] / floor[0], fused[0] / again[0], 1 + B),)), flush=True)
        n = C * nt
        for B in (1, 2, 4):
            back = median_of(lambda i: ctx.score_return(bufs[0].data_ptr(), [snd.data_ptr() + 4 * n * b for b in range(B)], n, bufs[1].data_ptr(), stream=s))
            print(line % ((label + ": the return kernel, B = %d (%.0f MB read, %.0f MB written)" % (B, (1 + B) * n * 4 / 1e6, n * 4 / 1e6),) + back + ("",)), flush=True)
        med, best = timed(lambda: ctx.fill(bufs[1].data_ptr(), n, 0.0, s), stream, reps)
        print(line % (label + ": dusp_fill_device over %.0f MB" % (n * 4 / 1e6), med, best, ""), flush=True)
        del bufs, snd
    del rows

    def echo(x):
        e = d.Sum(x, 0)
        e.B = d.Multiply(d.Delay(e, 300.25, 2048), 0.5)
        return e

    bus = ctx.build(descriptor.extract(echo(d.MasterInput())).words)
    for label, kw in (("no buses", {}), ("one echo bus, 300.25 samples", dict(buses=[(bus, None)], sends=levels[:1]))):
        times, kernel = [], []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            res = ctx.render_score_parts([(prog, nv, V, params)], np.zeros(V, dtype=np.uint32), onsets, nt, pinned=True, **kw)
            times.append((time.perf_counter() - t0) * 1e3)
            del res
            if kw:
                kernel.append(bus.last_kernel_ms())
        shape = "   bus render alone median %8.3f ms   [%s]" % (float(np.median(kernel[1:])), bus.read_shape()) if kw else ""
        print("  render_score_parts, host clock, %-30s median %9.2f ms  fastest %9.2f%s" % (label, float(np.median(times[1:])), min(times[1:]), shape), flush=True)
    bus.close()
    prog.close()


def tracks(scale, ctxs, reps):
    import torch
    V, nv, nt = max(64, 8192 // scale), SR // 2, 60 * SR
    d.configure(SR)
    ctx = ctxs["default"]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def median_of(call):
        kernel = []
        for r in range(reps + 1):
            call()
            if r:
                kernel.append(ctx.score_last_ms()[0])
        return float(np.median(kernel)), min(kernel)

    print("tracks: one channel of %d samples (%.1f MB a timeline), kernels alone by HIP events (dusp_score_last_ms), median and fastest of %d after a warm-up"
          % (nt, nt * 4 / 1e6, reps), flush=True)
    line = "  %-66s median %8.3f ms  fastest %8.3f%s"
    bufs = [torch.randn(nt, dtype=torch.float32, device="cuda") for _ in range(9)]
    out, feeds = torch.empty(nt, dtype=torch.float32, device="cuda"), torch.empty((2, nt), dtype=torch.float32, device="cuda")
    rs = np.random.RandomState(4)
    faders, levels = rs.random_sample(8).astype(np.float32), rs.random_sample((2, 8)).astype(np.float32)
    torch.cuda.synchronize()
    fill = timed(lambda: ctx.fill(out.data_ptr(), nt, 0.0, s), stream, reps)
    print(line % (("dusp_fill_device over one timeline (%.1f MB written)" % (nt * 4 / 1e6),) + fill + ("",)), flush=True)
    for T in (2, 4, 8):
        ys = [b.data_ptr() for b in bufs[1:1 + T]]
        if T <= 4:
            back = median_of(lambda: ctx.score_return(bufs[0].data_ptr(), ys, nt, out.data_ptr(), stream=s))
            print(line % (("dusp_score_return_kernel, %d inputs (%.0f MB read, %.0f MB written)" % (1 + T, (1 + T) * nt * 4 / 1e6, nt * 4 / 1e6),) + back + ("",)), flush=True)
        for B in (0, 2):
            mixed = median_of(lambda: ctx.score_tracks_mix(bufs[0].data_ptr(), ys, nt, out.data_ptr(), faders[:T], levels[:B, :T] if B else None, feeds.data_ptr() if B else None, stream=s))
            mb = ((1 + T) * nt * 4 / 1e6, (1 + B) * nt * 4 / 1e6)
            print(line % (("the mix kernel, T = %d, B = %d, with faders (%.0f MB read, %.0f MB written)" % ((T, B) + mb),) + mixed +
                          ("   %.0f GB/s, x%.2f of the fill" % ((mb[0] + mb[1]) / mixed[0], mixed[0] / fill[0]),)), flush=True)
    del bufs, out, feeds
    # eight Filter tracks as ONE program of eight instances, beside the same Filter as a master (one instance a channel: the master
    # path is the parent commit's, unchanged)
    note = lambda k: d.Multiply(d.Osc(110.0 + k / 8), d.Ramp(nv, 1, 0).trigger())
    uni = descriptor.unify([descriptor.extract(note(k)) for k in (0, 1)])
    params = (110.0 + np.arange(V, dtype=np.float64) / 8).astype(np.float32).reshape(1, V)
    onsets = np.sort(np.random.RandomState(1).randint(0, nt - nv, V)).astype(np.int64)
    prog = ctx.build(uni.words)
    lowpass = ctx.build(descriptor.extract(d.Filter(d.MasterInput(), 1200)).words)
    track_of = (np.arange(V) % 8).astype(np.int32)
    print("  %d notes of %d samples over %d samples, one channel, host clock, median and fastest of %d after a warm-up" % (V, nv, nt, reps), flush=True)
    for label, kw in (("no tracks, no master", {}), ("Filter(x, 1200) as the master (one instance)", dict(master=(lowpass, None))),
                      ("eight Filter(x, 1200) tracks, ONE program of eight instances", dict(tracks=dict(n_tracks=8, track_of=track_of, programs=[(lowpass, list(range(8)), None)])))):
        times, kernel = [], []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            res = ctx.render_score_parts([(prog, nv, V, params)], np.zeros(V, dtype=np.uint32), onsets, nt, pinned=True, **kw)
            times.append((time.perf_counter() - t0) * 1e3)
            del res
            if kw:
                kernel.append(lowpass.last_kernel_ms())
        shape = "   Filter render alone median %8.3f ms   [%s]" % (float(np.median(kernel[1:])), lowpass.read_shape()) if kw else ""
        print("  render_score_parts, %-62s median %9.2f ms  fastest %9.2f%s" % (label, float(np.median(times[1:])), min(times[1:]), shape), flush=True)
    times = []
    for r in range(reps + 1):  # the way round without track programs: eight renders of the piece's timeline through the Filter as a master, one after the other
        t0 = time.perf_counter()
        for g in range(8):
            res = ctx.render_score_parts([(prog, nv, V, params)], np.zeros(V, dtype=np.uint32), onsets, nt, pinned=True, master=(lowpass, None))
            del res
        times.append((time.perf_counter() - t0) * 1e3)
    print("  render_score_parts, %-62s median %9.2f ms  fastest %9.2f" % ("eight calls with the Filter as the master, one after the other", float(np.median(times[1:])), min(times[1:])), flush=True)
    lowpass.close()
    prog.close()


def stems(scale, ctxs, reps):
    import torch
    V, nv, nt = max(64, 8192 // scale), SR // 2, 60 * SR
    T, B = 8, 2
    d.configure(SR)
    ctx = ctxs["default"]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def median_of(call):
        kernel = []
        for r in range(reps + 1):
            call()
            if r:
                kernel.append(ctx.score_last_ms()[0])
        return float(np.median(kernel)), min(kernel), max(kernel)

    print("stems: one channel of %d samples (%.1f MB a timeline), T = %d tracks with faders, B = %d buses; kernels alone by HIP events (dusp_score_last_ms), median, fastest and slowest of %d after a warm-up"
          % (nt, nt * 4 / 1e6, T, B, reps), flush=True)
    line = "  %-78s median %8.3f ms  fastest %8.3f  slowest %8.3f%s"
    bufs = [torch.randn(nt, dtype=torch.float32, device="cuda") for _ in range(1 + T)]
    out, feeds = torch.empty(nt, dtype=torch.float32, device="cuda"), torch.empty((B, nt), dtype=torch.float32, device="cuda")
    slots = torch.empty((1 + T, nt), dtype=torch.float32, device="cuda")
    rs = np.random.RandomState(4)
    faders, levels = rs.random_sample(T).astype(np.float32), rs.random_sample((B, T)).astype(np.float32)
    ys = [b.data_ptr() for b in bufs[1:]]
    torch.cuda.synchronize()
    mb = lambda read, written: (read * nt * 4 / 1e6, written * nt * 4 / 1e6)
    old = median_of(lambda: ctx.score_tracks_mix(bufs[0].data_ptr(), ys, nt, out.data_ptr(), faders, levels, feeds.data_ptr(), stream=s))
    print(line % (("dusp_score_tracks_kernel (%.0f MB read, %.0f MB written)" % mb(1 + T, 1 + B),) + old + ("",)), flush=True)
    new = median_of(lambda: ctx.score_stems_mix(bufs[0].data_ptr(), ys, nt, out.data_ptr(), slots.data_ptr(), faders, levels, feeds.data_ptr(), stream=s))
    print(line % (("dusp_score_stems_mix_kernel, 1 + T slots more (%.0f MB read, %.0f MB written)" % mb(1 + T, 1 + B + 1 + T),) + new + ("   x%.2f of the mix kernel" % (new[0] / old[0]),)), flush=True)
    wets = ys[:B]
    old = median_of(lambda: ctx.score_return(bufs[0].data_ptr(), wets, nt, out.data_ptr(), stream=s))
    print(line % (("dusp_score_return_kernel (%.0f MB read, %.0f MB written)" % mb(1 + B, 1),) + old + ("",)), flush=True)
    new = median_of(lambda: ctx.score_stems_return(bufs[0].data_ptr(), wets, nt, out.data_ptr(), slots.data_ptr() + 4 * nt, stream=s))
    print(line % (("dusp_score_stems_return_kernel, B slots more (%.0f MB read, %.0f MB written)" % mb(1 + B, 1 + B),) + new + ("   x%.2f of the return kernel" % (new[0] / old[0]),)), flush=True)
    new = median_of(lambda: ctx.score_stems_return(bufs[0].data_ptr(), wets, nt, out.data_ptr(), slots.data_ptr() + 4 * nt, slots.data_ptr(), stream=s))
    print(line % (("dusp_score_stems_return_kernel, the direct slot too (%.0f MB read, %.0f MB written)" % mb(1 + B, 2 + B),) + new + ("   x%.2f of the return kernel" % (new[0] / old[0]),)), flush=True)
    del bufs, out, feeds, slots
    # the whole call: eight fader groups, two stateless buses (a gain each), no master
    note = lambda k: d.Multiply(d.Osc(110.0 + k / 8), d.Ramp(nv, 1, 0).trigger())
    uni = descriptor.unify([descriptor.extract(note(k)) for k in (0, 1)])
    params = (110.0 + np.arange(V, dtype=np.float64) / 8).astype(np.float32).reshape(1, V)
    onsets = np.sort(np.random.RandomState(1).randint(0, nt - nv, V)).astype(np.int64)
    prog = ctx.build(uni.words)
    buses = [ctx.build(descriptor.extract(d.Multiply(d.MasterInput(), g)).words) for g in (0.5, 0.25)]
    track_of = (np.arange(V) % T).astype(np.int32)
    S = 1 + T + B

    def call(f, **kw):
        res = ctx.render_score_parts([(prog, nv, V, params)], np.zeros(V, dtype=np.uint32), onsets, nt, pinned=True, buses=[(b, None) for b in buses],
                                     tracks=dict(n_tracks=T, track_of=track_of, programs=[], faders=f, track_sends=levels), **kw)
        del res

    def host_clock(run):
        times = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            run()
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times[1:])), min(times[1:]), max(times[1:])

    print("  %d notes of %d samples over %d samples, one channel, planar f32 into pinned memory, host clock, median, fastest and slowest of %d after a warm-up" % (V, nv, nt, reps), flush=True)
    row = "  render_score_parts, %-70s median %9.2f ms  fastest %9.2f  slowest %9.2f%s"
    plain = host_clock(lambda: call(faders))
    print(row % (("eight fader groups, two buses, no stems (%.0f MB delivered)" % (nt * 4 / 1e6),) + plain + ("",)), flush=True)
    with_stems = host_clock(lambda: call(faders, stems=True))
    print(row % (("the same with stems: %d signals (%.0f MB delivered)" % (S + 1, (S + 1) * nt * 4 / 1e6),) + with_stems + ("   x%.2f of the call without" % (with_stems[0] / plain[0]),)), flush=True)
    single = [np.where(np.arange(T) == g, faders, 0).astype(np.float32) for g in range(T)] + [np.zeros(T, dtype=np.float32)] * (1 + B)  # (a track alone; the direct mix and each bus alone: no track)
    apart = host_clock(lambda: [call(f) for f in single])
    print(row % (("the %d single-stem calls it replaces, one after the other" % S,) + apart + ("   x%.2f of the call with stems" % (apart[0] / with_stems[0]),)), flush=True)
    for b in buses:
        b.close()
    prog.close()


def meters(scale, ctxs, reps):
    """--meters: the meter kernels alone, pass by pass, beside the peak kernel over the same block; the call with stems
    with and without meters.  Under DUSP_HIP_LIB naming a library from before the meters only the call with stems runs."""
    import torch
    V, nv, nt = max(64, 8192 // scale), SR // 2, 60 * SR // (1 if scale == 1 else 8)
    T, B = 8, 2
    S = 1 + T + B
    d.configure(SR)
    ctx = ctxs["default"]
    has = hasattr(ctx._L, "dusp_meter_device")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    three = lambda xs: (float(np.median(xs)), min(xs), max(xs))
    line = "  %-78s median %8.3f ms  fastest %8.3f  slowest %8.3f%s"
    for C in ((1, 2) if has else ()):
        block = torch.randn((S + 1, C, nt), dtype=torch.float32, device="cuda") * 0.1
        n_hops = -(-nt // ((SR + 5) // 10))
        sumsq, hops, peaks = torch.empty((S + 1, C), dtype=torch.float64, device="cuda"), torch.empty((S + 1, n_hops), dtype=torch.float64, device="cuda"), torch.empty(S + 1, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        print("meters: %d signals of %d channel(s) of %d samples (%.0f MB), hop %d, segments of %d samples; kernels alone by HIP events, median, fastest and slowest of %d after a warm-up"
              % (S + 1, C, nt, block.numel() * 4 / 1e6, (SR + 5) // 10, 480 if SR == 48000 else -1, reps), flush=True)
        whole, passes, peak = [], [], []
        for r in range(reps + 1):
            ctx.meter_device(block.data_ptr(), S + 1, C, nt, SR, sumsq.data_ptr(), hops.data_ptr(), stream=s)
            if r:
                whole.append(ctx.score_last_ms()[0])
                passes.append(ctx.meter_last_ms())
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                ctx.peak(block.data_ptr(), S + 1, C, nt, peaks.data_ptr(), stream=s)
                e1.record()
            e1.synchronize()
            if r:
                peak.append(e0.elapsed_time(e1))
        print(line % (("the meter kernels, all passes (dusp_meter_device)",) + three(whole) + ("",)), flush=True)
        for k, name in enumerate(("pass A: every segment from rest", "combine: one lane a row over its segments' states", "pass B: every segment from its true state, z^2 and x^2",
                                  "reduce: segments -> hops -> d_hops, d_sumsq")):
            print(line % (("  " + name,) + three([p[k] for p in passes]) + ("",)), flush=True)
        print(line % (("dusp_pcm_peak_kernel over the same block (reads the same bytes once)",) + three(peak) + ("   the meters are x%.1f of it" % (np.median(whole) / np.median(peak)),)), flush=True)
        again = hops.clone()
        ctx.meter_device(block.data_ptr(), S + 1, C, nt, SR, sumsq.data_ptr(), hops.data_ptr(), stream=s)
        stream.synchronize()
        print("  two runs, the same bits: %s" % bool(torch.equal(again.view(torch.int64), hops.view(torch.int64))), flush=True)
        del block, sumsq, hops, peaks
    # the whole call: stems' piece — eight fader groups, two stateless buses (a gain each), no master — at one channel, and panned into two
    note = lambda k: d.Multiply(d.Osc(110.0 + k / 8), d.Ramp(nv, 1, 0).trigger())
    uni = descriptor.unify([descriptor.extract(note(k)) for k in (0, 1)])
    params = (110.0 + np.arange(V, dtype=np.float64) / 8).astype(np.float32).reshape(1, V)
    onsets = np.sort(np.random.RandomState(1).randint(0, nt - nv, V)).astype(np.int64)
    prog = ctx.build(uni.words)
    buses = [ctx.build(descriptor.extract(d.Multiply(d.MasterInput(), g)).words) for g in (0.5, 0.25)]
    track_of = (np.arange(V) % T).astype(np.int32)
    rs = np.random.RandomState(4)
    faders, levels = rs.random_sample(T).astype(np.float32), rs.random_sample((B, T)).astype(np.float32)

    def call(**kw):
        res = ctx.render_score_parts([(prog, nv, V, params)], np.zeros(V, dtype=np.uint32), onsets, nt, pinned=True, buses=[(b, None) for b in buses],
                                     tracks=dict(n_tracks=T, track_of=track_of, programs=[], faders=faders, track_sends=levels), stems=True, **kw)
        return res

    def host_clock(run):
        times = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            res = run()
            times.append((time.perf_counter() - t0) * 1e3)
            del res
        return three(times[1:])

    row = "  render_score_parts with stems, %-58s median %9.2f ms  fastest %9.2f  slowest %9.2f%s"
    print("  %d notes of %d samples over %d samples, %d signals, planar f32 into pinned memory, host clock, median, fastest and slowest of %d after a warm-up; library: %s"
          % (V, nv, nt, S + 1, reps, os.environ.get("DUSP_HIP_LIB") or "this tree's"), flush=True)
    for name, kw in (("one channel", {}), ("two channels (pans)", dict(pans=np.linspace(-1, 1, V)))):
        plain = host_clock(lambda: call(**kw))
        print(row % ((name + ", no meters",) + plain + ("",)), flush=True)
        if has:
            metered = host_clock(lambda: call(meters=True, **kw))
            print(row % ((name + ", meters=True",) + metered + ("   +%.2f ms, x%.2f" % (metered[0] - plain[0], metered[0] / plain[0]),)), flush=True)
            _, got = call(meters=True, **kw)
            print("    lufs of the mix %.2f, of track0 %.2f; %d blocks" % (got["lufs"][-1], got["lufs"][1], got["momentary"].shape[1]), flush=True)
    for b in buses:
        b.close()
    prog.close()


def loudness(scale, ctxs, reps):
    """--loudness: the true-peak kernel alone beside the peak kernel and the meter passes over the same block; the
    call with stems and s16 frames with loudness=-16 beside the same call with meters=True, normalise=2; and the call with stems
    without any new option, which under DUSP_HIP_LIB naming the parent's library is the only leg that runs."""
    import torch
    V, nv, nt = max(64, 8192 // scale), SR // 2, 60 * SR // (1 if scale == 1 else 8)
    T, B = 8, 2
    S = 1 + T + B
    d.configure(SR)
    ctx = ctxs["default"]
    has = hasattr(ctx._L, "dusp_true_peak_device")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    three = lambda xs: (float(np.median(xs)), min(xs), max(xs))
    line = "  %-78s median %8.3f ms  fastest %8.3f  slowest %8.3f%s"
    for C in ((1, 2) if has else ()):
        block = torch.randn((S + 1, C, nt), dtype=torch.float32, device="cuda") * 0.1
        n_hops = -(-nt // ((SR + 5) // 10))
        sumsq, hops, peaks = torch.empty((S + 1, C), dtype=torch.float64, device="cuda"), torch.empty((S + 1, n_hops), dtype=torch.float64, device="cuda"), torch.empty(S + 1, dtype=torch.float32, device="cuda")
        words = torch.empty((S + 1, C), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        print("loudness: %d signals of %d channel(s) of %d samples (%.0f MB) at %d Hz, F = 4, tiles of %d positions; kernels alone by HIP events, median, fastest and slowest of %d after a warm-up"
              % (S + 1, C, nt, block.numel() * 4 / 1e6, SR, ctx.true_peak_tile(S + 1, C, nt, SR), reps), flush=True)
        tp, whole, passes, peak = [], [], [], []
        for r in range(reps + 1):
            ctx.true_peak_device(block.data_ptr(), S + 1, C, nt, SR, words.data_ptr(), stream=s)
            if r:
                tp.append(ctx.score_last_ms()[0])
        for r in range(reps + 1):
            ctx.meter_device(block.data_ptr(), S + 1, C, nt, SR, sumsq.data_ptr(), hops.data_ptr(), stream=s)
            if r:
                whole.append(ctx.score_last_ms()[0])
                passes.append(ctx.meter_last_ms())
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                ctx.peak(block.data_ptr(), S + 1, C, nt, peaks.data_ptr(), stream=s)
                e1.record()
            e1.synchronize()
            if r:
                peak.append(e0.elapsed_time(e1))
        flops = 2.0 * 52 * block.numel()
        print(line % (("dusp_true_peak_kernel<4> (dusp_true_peak_device; memset of the words included)",) + three(tp) +
                      ("   %.2f GFLOP of unfused f64: %.1f TFLOP/s; %.0f GB/s read" % (flops / 1e9, flops / np.median(tp) / 1e9, block.numel() * 4 / np.median(tp) / 1e6),)), flush=True)
        print(line % (("dusp_pcm_peak_kernel over the same block (reads the same bytes once)",) + three(peak) + ("   the true peak is x%.1f of it" % (np.median(tp) / np.median(peak)),)), flush=True)
        print(line % (("the meter kernels, all passes (dusp_meter_device)",) + three(whole) + ("   the true peak is x%.2f of them" % (np.median(tp) / np.median(whole)),)), flush=True)
        for k, name in ((0, "pass A: every segment from rest"), (2, "pass B: every segment from its true state, z^2 and x^2")):
            print(line % (("  " + name,) + three([p[k] for p in passes]) + ("",)), flush=True)
        again = words.clone()
        ctx.true_peak_device(block.data_ptr(), S + 1, C, nt, SR, words.data_ptr(), stream=s)
        stream.synchronize()
        print("  two runs, the same bits: %s; the largest true peak %.4f, the largest sample %.4f" % (bool(torch.equal(again, words)), float(words.view(torch.float64).max()), float(block.abs().max())),
              flush=True)
        del block, sumsq, hops, peaks, words
    # the whole call: stems' piece — eight fader groups, two stateless buses (a gain each), no master — at one channel, and panned into two
    note = lambda k: d.Multiply(d.Osc(110.0 + k / 8), d.Ramp(nv, 1, 0).trigger())
    uni = descriptor.unify([descriptor.extract(note(k)) for k in (0, 1)])
    params = (110.0 + np.arange(V, dtype=np.float64) / 8).astype(np.float32).reshape(1, V)
    onsets = np.sort(np.random.RandomState(1).randint(0, nt - nv, V)).astype(np.int64)
    prog = ctx.build(uni.words)
    buses = [ctx.build(descriptor.extract(d.Multiply(d.MasterInput(), g)).words) for g in (0.5, 0.25)]
    track_of = (np.arange(V) % T).astype(np.int32)
    rs = np.random.RandomState(4)
    faders, levels = rs.random_sample(T).astype(np.float32), rs.random_sample((B, T)).astype(np.float32)

    def call(**kw):
        return ctx.render_score_parts([(prog, nv, V, params)], np.zeros(V, dtype=np.uint32), onsets, nt, pinned=True, buses=[(b, None) for b in buses],
                                      tracks=dict(n_tracks=T, track_of=track_of, programs=[], faders=faders, track_sends=levels), stems=True, **kw)

    def host_clock(run):
        times = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            res = run()
            times.append((time.perf_counter() - t0) * 1e3)
            del res
        return three(times[1:])

    row = "  render_score_parts with stems, %-66s median %9.2f ms  fastest %9.2f  slowest %9.2f%s"
    print("  %d notes of %d samples over %d samples, %d signals, into pinned memory, host clock, median, fastest and slowest of %d after a warm-up; library: %s"
          % (V, nv, nt, S + 1, reps, os.environ.get("DUSP_HIP_LIB") or "this tree's"), flush=True)
    for name, kw in (("one channel", {}), ("two channels (pans)", dict(pans=np.linspace(-1, 1, V)))):
        plain = host_clock(lambda: call(**kw))
        print(row % ((name + ", planar f32, no new option",) + plain + ("",)), flush=True)
        frames = host_clock(lambda: call(format="s16", normalise=2, **kw))
        print(row % ((name + ", s16, normalise=2, no new option",) + frames + ("",)), flush=True)
        if has:
            metered = host_clock(lambda: call(format="s16", normalise=2, meters=True, **kw))
            print(row % ((name + ", s16, normalise=2, meters=True",) + metered + ("",)), flush=True)
            peaked = host_clock(lambda: call(format="s16", normalise=2, true_peak=True, **kw))
            print(row % ((name + ", s16, normalise=2, true_peak=True",) + peaked + ("   +%.2f ms, x%.3f of meters=True" % (peaked[0] - metered[0], peaked[0] / metered[0]),)), flush=True)
            loud = host_clock(lambda: call(format="s16", loudness=-16.0, **kw))
            print(row % ((name + ", s16, loudness=-16",) + loud + ("   +%.2f ms, x%.3f of meters=True, normalise=2" % (loud[0] - metered[0], loud[0] / metered[0]),)), flush=True)
            _, got = call(format="s16", loudness=-16.0, **kw)
            print("    lufs of the mix %.2f, largest true peak %.4f, level %r, gain %.6f: the mix leaves at %.2f LUFS, the largest true peak at %.2f dBTP"
                  % (got["lufs"][-1], got["true_peak"].max(), got["level"], got["gain"], got["lufs"][-1] + 20 * np.log10(got["gain"]), 20 * np.log10(got["true_peak"].max() * got["gain"])), flush=True)
    for b in buses:
        b.close()
    prog.close()


def limiter(scale, ctxs, reps):
    """--limiter: the limiter's envelope kernel beside the true-peak kernel and its gain / apply kernel beside the peak
    kernel over the same block, at a window of 5 ms and at the longest window; the call with stems and s16 frames at a loudness target
    with the limiter engaged and not engaged beside the same call without it, which under DUSP_HIP_LIB naming the parent's library is
    the only leg that runs."""
    import torch
    V, nv, nt = max(64, 8192 // scale), SR // 2, 60 * SR // (1 if scale == 1 else 8)
    T, B = 8, 2
    S = 1 + T + B
    d.configure(SR)
    ctx = ctxs["default"]
    has = hasattr(ctx._L, "dusp_limit_device")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    three = lambda xs: (float(np.median(xs)), min(xs), max(xs))
    line = "  %-78s median %8.3f ms  fastest %8.3f  slowest %8.3f%s"
    for C in ((1, 2) if has else ()):
        source = torch.randn((S + 1, C, nt), dtype=torch.float32, device="cuda") * 0.1
        block, peaks, words = source.clone(), torch.empty(S + 1, dtype=torch.float32, device="cuda"), torch.empty((S + 1, C), dtype=torch.int64, device="cuda")
        word = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        print("limiter: %d signals of %d channel(s) of %d samples (%.0f MB) at %d Hz, F = 4; kernels alone by HIP events, median, fastest and slowest of %d after a warm-up"
              % (S + 1, C, nt, block.numel() * 4 / 1e6, SR, reps), flush=True)
        tp, peak = [], []
        for r in range(reps + 1):
            ctx.true_peak_device(source.data_ptr(), S + 1, C, nt, SR, words.data_ptr(), stream=s)
            if r:
                tp.append(ctx.score_last_ms()[0])
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                ctx.peak(source.data_ptr(), S + 1, C, nt, peaks.data_ptr(), stream=s)
                e1.record()
            e1.synchronize()
            if r:
                peak.append(e0.elapsed_time(e1))
        print(line % (("dusp_true_peak_kernel<4> over the block (the same f64 work, no division)",) + three(tp) + ("",)), flush=True)
        print(line % (("dusp_pcm_peak_kernel over the block (reads it once)",) + three(peak) + ("",)), flush=True)
        threshold = 0.2  # (two standard deviations of the noise: a few samples in a hundred lie above it)
        for L in (240, 4096):
            envelope, apply, first = [], [], None
            for r in range(reps + 1):
                with torch.cuda.stream(stream):
                    block.copy_(source)  # (the limiter works in place: every run limits the same signals)
                ctx.limit_device(block.data_ptr(), S + 1, C, nt, SR, threshold, L, d_smallest=word.data_ptr(), stream=s)
                if r:
                    ms = ctx.limit_last_ms()
                    envelope.append(ms[0]), apply.append(ms[1])
                if first is None:
                    with torch.cuda.stream(stream):
                        first = block.clone()
                stream.synchronize()
            flops = 2.0 * 52 * block.numel()
            print("  window %d samples, tiles of %d samples, reduction %.4f, two runs the same bits: %s" % (L, ctx.limit_tile(nt, L), int(word.item()) / float(L * (1 << 30)), bool(torch.equal(first, block))),
                  flush=True)
            print(line % (("  dusp_limit_envelope_kernel<4>",) + three(envelope) +
                          ("   %.1f TFLOP/s of unfused f64; x%.2f of the true-peak kernel" % (flops / np.median(envelope) / 1e9, np.median(envelope) / np.median(tp)),)), flush=True)
            print(line % (("  dusp_limit_apply_kernel (reads and writes the block once)",) + three(apply) +
                          ("   %.0f GB/s moved; x%.2f of the peak kernel" % (2 * block.numel() * 4 / np.median(apply) / 1e6, np.median(apply) / np.median(peak)),)), flush=True)
        del source, block, peaks, words
    # the whole call: stems' piece — eight fader groups, two stateless buses (a gain each), no master — at one channel, and panned into two
    note = lambda k: d.Multiply(d.Osc(110.0 + k / 8), d.Ramp(nv, 1, 0).trigger())
    uni = descriptor.unify([descriptor.extract(note(k)) for k in (0, 1)])
    params = (110.0 + np.arange(V, dtype=np.float64) / 8).astype(np.float32).reshape(1, V)
    onsets = np.sort(np.random.RandomState(1).randint(0, nt - nv, V)).astype(np.int64)
    prog = ctx.build(uni.words)
    buses = [ctx.build(descriptor.extract(d.Multiply(d.MasterInput(), g)).words) for g in (0.5, 0.25)]
    track_of = (np.arange(V) % T).astype(np.int32)
    rs = np.random.RandomState(4)
    faders, levels = rs.random_sample(T).astype(np.float32), rs.random_sample((B, T)).astype(np.float32)

    def call(**kw):
        return ctx.render_score_parts([(prog, nv, V, params)], np.zeros(V, dtype=np.uint32), onsets, nt, pinned=True, buses=[(b, None) for b in buses],
                                      tracks=dict(n_tracks=T, track_of=track_of, programs=[], faders=faders, track_sends=levels), stems=True, **kw)

    def host_clock(run):
        times = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            res = run()
            times.append((time.perf_counter() - t0) * 1e3)
            del res
        return three(times[1:])

    row = "  render_score_parts with stems, %-66s median %9.2f ms  fastest %9.2f  slowest %9.2f%s"
    print("  %d notes of %d samples over %d samples, %d signals, into pinned memory, host clock, median, fastest and slowest of %d after a warm-up; library: %s"
          % (V, nv, nt, S + 1, reps, "another build's, named by DUSP_HIP_LIB" if os.environ.get("DUSP_HIP_LIB") else "this tree's"), flush=True)
    window = 240.0 / SR
    for name, kw in (("one channel", {}), ("two channels (pans)", dict(pans=np.linspace(-1, 1, V)))):
        frames = host_clock(lambda: call(format="s16", normalise=2, **kw))
        print(row % ((name + ", s16, normalise=2, no new option",) + frames + ("",)), flush=True)
        loud = host_clock(lambda: call(format="s16", loudness=-16.0, **kw))
        print(row % ((name + ", s16, loudness=-16",) + loud + ("",)), flush=True)
        _, got = call(format="s16", loudness=-16.0, **kw)
        # a target 6 dB above the one at which the largest true peak meets the ceiling: the limiter engages; 12 dB below that: it does not
        meets = got["lufs"][-1] + 20 * np.log10(10 ** (-1 / 20) / got["true_peak"].max())
        high, low = float(meets + 6.0), float(meets - 6.0)
        for target in (low, high):
            there = host_clock(lambda: call(format="s16", loudness=target, **kw))
            print(row % ((name + ", s16, loudness=%.2f" % target,) + there + ("",)), flush=True)
            if has:
                limited = host_clock(lambda: call(format="s16", loudness=target, limiter=True, limiter_window=window, **kw))
                _, did = call(format="s16", loudness=target, limiter=True, limiter_window=window, **kw)
                print(row % ((name + ", s16, loudness=%.2f, limiter=True: %s" % (target, "engaged" if did["limiter"]["engaged"] else "not engaged"),) + limited +
                             ("   +%.2f ms, x%.3f of the call without" % (limited[0] - there[0], limited[0] / there[0]),)), flush=True)
                print("    threshold %.4f against a largest true peak of %.4f, reduction %.4f; gain %.4f, the mix leaves at %.2f LUFS, the largest true peak at %.2f dBTP"
                      % (did["limiter"]["threshold"], did["limiter"]["true_peak_in"], did["limiter"]["reduction"], did["gain"], did["lufs"][-1] + 20 * np.log10(did["gain"]),
                         20 * np.log10(did["true_peak"].max() * did["gain"])), flush=True)
    for b in buses:
        b.close()
    prog.close()


def limiter_release(scale, ctxs, reps):
    """--limiter-release: the launches of a limiter call with a release of its own — envelope, hold, release, mean / apply —
    by HIP events at a window of 5 ms and releases of 50 ms, 500 ms and 2^22 samples, beside dusp_limit_apply_kernel at the same window in
    the same run; the call with stems and s16 frames at a loudness target with the limiter engaged, with and without a release; and the
    calls without the option, the only leg that runs under DUSP_HIP_LIB naming the parent's library."""
    import torch
    V, nv, nt = max(64, 8192 // scale), SR // 2, 60 * SR // (1 if scale == 1 else 8)
    T, B = 8, 2
    S = 1 + T + B
    d.configure(SR)
    ctx = ctxs["default"]
    has = hasattr(ctx._L, "dusp_limit_release_device")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    three = lambda xs: (float(np.median(xs)), min(xs), max(xs))
    line = "  %-78s median %8.3f ms  fastest %8.3f  slowest %8.3f%s"
    L = 240
    for C in ((1, 2) if has else ()):
        source = torch.randn((S + 1, C, nt), dtype=torch.float32, device="cuda") * 0.1
        block, word = source.clone(), torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        print("limiter release: %d signals of %d channel(s) of %d samples (%.0f MB) at %d Hz, F = 4, window %d, tiles of %d; launches by HIP events, median, fastest and slowest of %d after a warm-up"
              % (S + 1, C, nt, block.numel() * 4 / 1e6, SR, L, ctx.limit_release_tile(nt, L, 2400), reps), flush=True)
        threshold = 0.2  # (two standard deviations of the noise: a few samples in a hundred lie above it)
        envelope, apply = [], []
        for r in range(reps + 1):
            with torch.cuda.stream(stream):
                block.copy_(source)  # (the limiter works in place: every run limits the same signals)
            ctx.limit_device(block.data_ptr(), S + 1, C, nt, SR, threshold, L, d_smallest=word.data_ptr(), stream=s)
            if r:
                ms = ctx.limit_last_ms()
                envelope.append(ms[0]), apply.append(ms[1])
            stream.synchronize()
        moved = 2 * block.numel() * 4
        print(line % (("no release: dusp_limit_envelope_kernel<4>",) + three(envelope) + ("",)), flush=True)
        print(line % (("no release: dusp_limit_apply_kernel, the yardstick (%d bytes a sample of signals)" % (moved // nt),) + three(apply) +
                      ("   %.0f GB/s moved; reduction %.4f" % (moved / np.median(apply) / 1e6, int(word.item()) / float(L * (1 << 30))),)), flush=True)
        for R in (2400, 24000, 1 << 22):
            parts, first = [[], [], [], []], None
            for r in range(reps + 1):
                with torch.cuda.stream(stream):
                    block.copy_(source)
                ctx.limit_release_device(block.data_ptr(), S + 1, C, nt, SR, threshold, L, R, d_smallest=word.data_ptr(), stream=s)
                if r:
                    for k, ms in enumerate(ctx.limit_release_last_ms()):
                        parts[k].append(ms)
                if first is None:
                    with torch.cuda.stream(stream):
                        first = block.clone()
                stream.synchronize()
            print("  release %d samples, d = %d, reduction %.4f, two runs the same bits: %s" % (R, -(-(1 << 30) // R), int(word.item()) / float(L * (1 << 30)), bool(torch.equal(first, block))), flush=True)
            for k, name in enumerate(("dusp_limit_envelope_kernel<4>", "dusp_limit_hold_kernel (reads q, writes m: 8 bytes a sample)", "dusp_limit_release_kernel (reads m, writes held: 8 bytes a sample)",
                                      "dusp_limit_mean_apply_kernel (reads and writes the block once)")):
                extra = "" if k == 0 else "   x%.2f of the apply kernel" % (np.median(parts[k]) / np.median(apply))
                print(line % (("  " + name,) + three(parts[k]) + (extra,)), flush=True)
            added = np.median(parts[1]) + np.median(parts[2]) + np.median(parts[3]) - np.median(apply)
            print("    the three launches cost %.3f ms more than the apply kernel they stand for, x%.2f of it" % (added, added / np.median(apply)), flush=True)
        del source, block
    # the whole call: stems' piece — eight fader groups, two stateless buses (a gain each), no master — at one channel, and panned into two
    note = lambda k: d.Multiply(d.Osc(110.0 + k / 8), d.Ramp(nv, 1, 0).trigger())
    uni = descriptor.unify([descriptor.extract(note(k)) for k in (0, 1)])
    params = (110.0 + np.arange(V, dtype=np.float64) / 8).astype(np.float32).reshape(1, V)
    onsets = np.sort(np.random.RandomState(1).randint(0, nt - nv, V)).astype(np.int64)
    prog = ctx.build(uni.words)
    buses = [ctx.build(descriptor.extract(d.Multiply(d.MasterInput(), g)).words) for g in (0.5, 0.25)]
    track_of = (np.arange(V) % T).astype(np.int32)
    rs = np.random.RandomState(4)
    faders, levels = rs.random_sample(T).astype(np.float32), rs.random_sample((B, T)).astype(np.float32)

    def call(**kw):
        return ctx.render_score_parts([(prog, nv, V, params)], np.zeros(V, dtype=np.uint32), onsets, nt, pinned=True, buses=[(b, None) for b in buses],
                                      tracks=dict(n_tracks=T, track_of=track_of, programs=[], faders=faders, track_sends=levels), stems=True, **kw)

    def host_clock(run):
        times = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            res = run()
            times.append((time.perf_counter() - t0) * 1e3)
            del res
        return three(times[1:])

    row = "  render_score_parts with stems, %-72s median %9.2f ms  fastest %9.2f  slowest %9.2f%s"
    print("  %d notes of %d samples over %d samples, %d signals, into pinned memory, host clock, median, fastest and slowest of %d after a warm-up; library: %s"
          % (V, nv, nt, S + 1, reps, "another build's, named by DUSP_HIP_LIB" if os.environ.get("DUSP_HIP_LIB") else "this tree's"), flush=True)
    window = 240.0 / SR
    for name, kw in (("one channel", {}), ("two channels (pans)", dict(pans=np.linspace(-1, 1, V)))):
        frames = host_clock(lambda: call(format="s16", normalise=2, **kw))
        print(row % ((name + ", s16, normalise=2, no new option",) + frames + ("",)), flush=True)
        loud = host_clock(lambda: call(format="s16", loudness=-16.0, **kw))
        print(row % ((name + ", s16, loudness=-16",) + loud + ("",)), flush=True)
        _, got = call(format="s16", loudness=-16.0, **kw)
        high = float(got["lufs"][-1] + 20 * np.log10(10 ** (-1 / 20) / got["true_peak"].max()) + 6.0)  # (6 dB above where the largest true peak meets the ceiling: engaged)
        there = host_clock(lambda: call(format="s16", loudness=high, limiter=True, limiter_window=window, **kw))
        print(row % ((name + ", s16, loudness=%.2f, limiter=True, engaged" % high,) + there + ("",)), flush=True)
        for seconds in ((0.05, 0.5) if has else ()):
            released = host_clock(lambda: call(format="s16", loudness=high, limiter=True, limiter_window=window, limiter_release=seconds, **kw))
            _, did = call(format="s16", loudness=high, limiter=True, limiter_window=window, limiter_release=seconds, **kw)
            print(row % ((name + ", ... and limiter_release=%.2f (%d samples)" % (seconds, did["limiter"]["release"]),) + released +
                         ("   %+.2f ms, x%.3f of the call without a release" % (released[0] - there[0], released[0] / there[0]),)), flush=True)
            print("    reduction %.4f; gain %.4f, the mix leaves at %.2f LUFS, the largest true peak at %.2f dBTP"
                  % (did["limiter"]["reduction"], did["gain"], did["lufs"][-1] + 20 * np.log10(did["gain"]), 20 * np.log10(did["true_peak"].max() * did["gain"])), flush=True)
    for b in buses:
        b.close()
    prog.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="abcd", help="dense cases to run; add p for the piece")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide every voice count by this (a quick look)")
    ap.add_argument("--pan", action="store_true", help="the pan leg alone, over the dense cases named by --cases")
    ap.add_argument("--frac", action="store_true", help="the sub-sample-onset leg alone, over the dense cases named by --cases")
    ap.add_argument("--space", action="store_true", help="the Space-placement leg alone, over the dense cases named by --cases")
    ap.add_argument("--stereo", action="store_true", help="the stereo-piece leg alone, over the dense cases named by --cases")
    ap.add_argument("--master", action="store_true", help="the master-bus leg alone: the piece with and without a master")
    ap.add_argument("--sends", action="store_true", help="the effect-send leg alone: the send and return kernels, and the piece with and without a bus")
    ap.add_argument("--tracks", action="store_true", help="the tracks leg alone: the mix kernel beside the fill and the return kernel, and eight Filter tracks as one program")
    ap.add_argument("--stems", action="store_true", help="the stems leg alone: the stems mix and return kernels beside the kernels they extend, and the piece with and without stems")
    ap.add_argument("--meters", action="store_true", help="the meters leg alone: the meter kernels pass by pass beside the peak kernel, and the piece with stems with and without meters")
    ap.add_argument("--loudness", action="store_true", help="the loudness leg alone: the true-peak kernel beside the peak kernel and the meter passes, and the piece with stems delivered at a loudness target")
    ap.add_argument("--limiter", action="store_true", help="the limiter leg alone: its two kernels beside the true-peak and peak kernels, and the piece with stems at a loudness target with and without the limiter")
    ap.add_argument("--limiter-release", action="store_true", help="the limiter's release alone: its launches beside the apply kernel, and the piece with stems at a loudness target with and without a release")
    a = ap.parse_args()
    os.environ["DUSP_WAVE_JIT"] = "2"  # wait for compiled kernels
    ctxs = {"default": context(), "dword8": context(DUSP_MIX_WIDTH=1, DUSP_MIX_DEPTH=8), "one_block": context(DUSP_SCORE_PLAN_KB=1), "log": context(DUSP_JIT_LOG=2)}
    if a.master:
        return master(a.scale, ctxs, a.reps)
    if a.sends:
        return sends(a.scale, ctxs, a.reps)
    if a.tracks:
        return tracks(a.scale, ctxs, a.reps)
    if a.stems:
        return stems(a.scale, ctxs, a.reps)
    if a.meters:
        return meters(a.scale, ctxs, a.reps)
    if a.loudness:
        return loudness(a.scale, ctxs, a.reps)
    if a.limiter:
        return limiter(a.scale, ctxs, a.reps)
    if a.limiter_release:
        return limiter_release(a.scale, ctxs, a.reps)
    for key in a.cases:
        if key in DENSE:
            (stereo if a.stereo else space if a.space else frac if a.frac else pan if a.pan else dense)(key, a.scale, ctxs, a.reps)
    if "p" in a.cases and not a.pan and not a.frac and not a.space and not a.stereo:
        piece(a.scale, ctxs, a.reps)


if __name__ == "__main__":
    main()
