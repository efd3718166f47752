#!/usr/bin/env python3
"""Device-side PCM delivery, measured (run by hand on the GPU; the output is kept as profiles/pcm_encode.txt).

Device times (HIP events on the launch stream) for 1- and 2-channel batches that fill the chip and do not fit the Infinity
Cache: dusp_interleave_device (the baseline: code this feature does not touch; a 1-channel batch is its device-to-device copy),
dusp_encode_device to s16 and s24 without normalisation, dusp_peak_device alone, and peak + encode.  The variants are timed in
turn, round after round, so that whatever else shares the machine hits all of them alike; each line gives the median, the
fastest round and the spread (10th to 90th percentile) of its own rounds.

Then the host-inclusive wall time of Program.render(interleaved=True) against Program.render_pcm("s16") into pinned memory, for a
batch of about 1 GB of f32: what a caller who wants a 16-bit file waits for.

Read the ratios against the bytes moved per sample: interleave 4 + 4, s16 4 + 2 (0.75 of interleave), s24 4 + 3, peak 4,
peak + s16 4 + 4 + 2 (1.25 of interleave); across the link f32 4, s16 2 (0.5).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dusp_amd as d  # noqa: E402
from dusp_amd import descriptor, runtime  # noqa: E402


def device_part(ctx, n_inst, n_ch, n, rounds, warmup):
    import torch
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(n_ch)
    x = torch.randn((n_inst, n_ch, n), generator=gen, dtype=torch.float32, device="cuda") * 0.7
    out = torch.empty(n_inst * n_ch * n * 4, dtype=torch.uint8, device="cuda")
    peaks = torch.empty(n_inst, dtype=torch.float32, device="cuda")
    xp, op, pp = x.data_ptr(), out.data_ptr(), peaks.data_ptr()
    samples = n_inst * n_ch * n
    variants = [
        ("interleave f32 (baseline)", 8, lambda: ctx.interleave(xp, n_inst, n_ch, n, op, s)),
        ("encode s16, normalise 0", 6, lambda: ctx.encode(xp, n_inst, n_ch, n, op, "s16", 0, None, s)),
        ("encode s24, normalise 0", 7, lambda: ctx.encode(xp, n_inst, n_ch, n, op, "s24", 0, None, s)),
        ("peak alone", 4, lambda: ctx.peak(xp, n_inst, n_ch, n, pp, s)),
        ("peak + encode s16, normalise 2", 10, lambda: (ctx.peak(xp, n_inst, n_ch, n, pp, s), ctx.encode(xp, n_inst, n_ch, n, op, "s16", 2, pp, s))),
        ("peak + encode s24, normalise 2", 11, lambda: (ctx.peak(xp, n_inst, n_ch, n, pp, s), ctx.encode(xp, n_inst, n_ch, n, op, "s24", 2, pp, s))),
    ]
    times = [[] for _ in variants]
    torch.cuda.synchronize()
    for r in range(warmup + rounds):
        for k, (_, _, call) in enumerate(variants):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            if r >= warmup:
                times[k].append(a.elapsed_time(b))
    print("%d instances x %d channel(s) x %d samples = %.0f MB of f32, %d rounds after %d warm-up rounds" % (n_inst, n_ch, n, samples * 4 / 1e6, rounds, warmup))
    base = float(np.median(times[0]))
    for (name, bytes_per_sample, _), t in zip(variants, times):
        t = np.array(t)
        med, lo, hi = float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))
        print("  %-32s median %8.3f ms  fastest %8.3f  p10-p90 %8.3f - %8.3f  %6.2f TB/s of %2d B/sample  x%.3f of interleave (bytes: x%.3f)"
              % (name, med, float(t.min()), lo, hi, samples * bytes_per_sample / med / 1e9, bytes_per_sample, med / base, bytes_per_sample / 8), flush=True)
    spread = (float(np.percentile(times[0], 90)) - float(np.percentile(times[0], 10))) / base
    s16 = float(np.median(times[1]))
    print("  criterion: encode s16 / interleave = %.3f; the interleave timings spread by %.1f%% (p10-p90 over the median): %s"
          % (s16 / base, 100 * spread, "not slower" if s16 <= base * (1 + spread) else "SLOWER than interleave beyond its spread"), flush=True)


def host_part(ctx, sr, voices, seconds, reps):
    n = sr * seconds
    uni = descriptor.unify([descriptor.extract(d.Multiply(d.Multiply(d.Osc(10 * k), d.Ramp(n, 1, 0).trigger()), [0.9, 0.4])) for k in (1, 2)])
    assert uni.n_params == 1  # the oscillator's frequency
    params = (10.0 * np.arange(1, voices + 1)).astype(np.float32).reshape(1, voices)
    prog = ctx.build(uni.words)
    calls = [("render(interleaved=True), f32", 4, lambda: prog.render(n, voices, params, interleaved=True, pinned=True)),
             ('render_pcm("s16", normalise=0)', 2, lambda: prog.render_pcm(n, voices, params, format="s16", normalise=0, pinned=True)[0]),
             ('render_pcm("s16", normalise=2)', 2, lambda: prog.render_pcm(n, voices, params, format="s16", normalise=2, pinned=True)[0]),
             ('render_pcm("s24", normalise=2)', 3, lambda: prog.render_pcm(n, voices, params, format="s24", normalise=2, pinned=True)[0])]
    times = [[] for _ in calls]
    for r in range(reps + 2):
        for k, (_, _, call) in enumerate(calls):
            t0 = time.perf_counter()
            res = call()
            dt = time.perf_counter() - t0
            del res  # (back to the pinned pool: the next call of this size reuses the block)
            if r >= 2:
                times[k].append(dt)
    samples = voices * prog.n_out_channels * n
    print("host-inclusive wall time into pinned memory: %d voices x %d channels x %d s = %.0f MB of f32, %d calls each after 2 warm-up calls"
          % (voices, prog.n_out_channels, seconds, samples * 4 / 1e6, reps))
    base = float(np.median(times[0]))
    for (name, b, _), t in zip(calls, times):
        med = float(np.median(t))
        print("  %-32s median %8.2f ms  fastest %8.2f  slowest %8.2f  %6.2f GB/s across the link  x%.3f of f32 (bytes: x%.3f)"
              % (name, med * 1e3, min(t) * 1e3, max(t) * 1e3, samples * b / med / 1e9, med / base, b / 4), flush=True)
    prog.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", type=int, default=128)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--voices", type=int, default=512)
    ap.add_argument("--seconds", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    sr = 48000
    d.configure(sr)
    ctx = runtime.Context(0, sr)
    for n_ch in (1, 2):
        device_part(ctx, a.instances, n_ch, a.samples, a.rounds, a.warmup)
    if not a.skip_host:
        host_part(ctx, sr, a.voices, a.seconds, a.host_reps)


if __name__ == "__main__":
    main()
