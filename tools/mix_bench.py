#!/usr/bin/env python3
"""The device-side mix, measured (run by hand on the GPU; the output is kept as profiles/mix_chain.txt).

Four batches whose mix used to mean downloading every voice:
  a  8192 feedback voices (BASELINE configs[3]) x 10 s
  b  1024 Multiply(Osc(10k), Ramp) voices x 60 s
  c  16384 filtered oscillators x 1 s
  d  65536 enveloped oscillators x 1 s  (many voices, a grid that is narrow in time)

For each, with HIP events on the launch stream:
  * the yardstick: Program.render_device of the same voices into a preallocated buffer, WITHOUT the mix;
  * dusp_mix_device over that buffer, all instances in one launch, by the launcher's own choice of width and with one float
    (DUSP_MIX_WIDTH=1) and four floats (=4) a lane: the time, the bytes read per second, and how far that is from the
    6.29 TB/s a float4 copy reaches on this part (the mix reads every voice once and writes one voice's worth); the dword form
    with 8 and with 32 rows in flight per lane (DUSP_MIX_DEPTH);
  * the same kernel over one tile's worth of instances that the render has just written, for tiles of 64 MiB to 2 GiB: do tiles
    that fit the 256 MiB Infinity Cache read faster than the HBM rate?
and, on the host's clock, Program.render_mix — upload, tiles of render + mix, download of one voice's worth — for default
tiles of 64 MiB, 128 MiB, 512 MiB and 2 GiB of PCM (DUSP_MIX_TILE_MB; cases a and b unless --sweep-all) and for the library's own
default tile, the batch that fills the chip.

Every variant is timed `--reps` times after a warm-up call; lines give the median and the fastest.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dusp_amd as d  # noqa: E402
from dusp_amd import descriptor, runtime  # noqa: E402

SR = 48000
COPY_RATE = 6.29e12  # bytes / s, float4 copy
TILES_MB = (64, 128, 512, 2048)


def context(**knobs):
    """a context created under the given DUSP_* knobs (read once, in dusp_ctx_create)"""
    saved = {k: os.environ.get(k) for k in knobs}
    os.environ.update({k: str(v) for k, v in knobs.items()})
    try:
        return runtime.Context(0, SR)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def feedback(k):
    s = d.Sum(d.Osc(110 + k / 64), 0)
    f = d.Filter(d.Delay(s, 480, 4096), 2000)
    s.B = d.Multiply(f, 0.5)
    return f


def cases(scale):
    """name -> (voice builder over k, parameter column over k, voices, samples)"""
    v = lambda n: max(64, n // scale)
    return {
        "a": ("feedback voices x 10 s", feedback, lambda k: 110 + k / 64.0, v(8192), 10 * SR),
        "b": ("Multiply(Osc(10k), Ramp) x 60 s", lambda k: d.Multiply(d.Osc(10.0 * (k + 1)), d.Ramp(60 * SR, 1, 0).trigger()), lambda k: 10.0 * (k + 1), v(1024), 60 * SR),
        "c": ("filter(osc) x 1 s", lambda k: d.Filter(d.Osc(110 + k / 4, "saw"), 2000), lambda k: 110 + k / 4.0, v(16384), SR),
        "d": ("Multiply(Osc, Ramp) x 1 s", lambda k: d.Multiply(d.Osc(20 + k / 8), d.Ramp(SR, 1, 0).trigger()), lambda k: 20 + k / 8.0, v(65536), SR),
    }


def timed(call, stream, reps):
    import torch
    out = []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        if r:
            out.append(a.elapsed_time(b))
    return float(np.median(out)), float(min(out))


def run_case(key, spec, ctxs, tile_ctxs, reps):
    import torch
    title, build, column, V, n = spec
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    d.configure(SR)
    uni = descriptor.unify([descriptor.extract(build(k)) for k in (0, 1)])
    assert uni.n_params == 1, uni.n_params
    params = column(np.arange(V, dtype=np.float64)).astype(np.float32).reshape(1, V)
    prog = ctxs["by grid"].build(uni.words)
    C = prog.n_out_channels
    row_bytes = C * n * 4
    print("case %s: %d %s = %.2f GB of f32, engine %s" % (key, V, title, V * row_bytes / 1e9, prog.engine), flush=True)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    out = torch.empty((V, C, n), dtype=torch.float32, device="cuda")
    acc = torch.empty((C, n), dtype=torch.float32, device="cuda")
    dp = torch.from_numpy(params).cuda()
    torch.cuda.synchronize()
    med, best = timed(lambda: prog.render_device(n, V, dp.data_ptr(), out.data_ptr(), s), stream, reps)
    print("  render without the mix (yardstick)      median %9.3f ms  fastest %9.3f   [%s]" % (med, best, prog.read_shape()), flush=True)
    t_render = med
    floor = V * row_bytes / COPY_RATE * 1e3
    for label, ctx in ctxs.items():
        med, best = timed(lambda: ctx.mix(out.data_ptr(), V, C, n, acc.data_ptr(), None, None, False, s), stream, reps)
        rate = (V + 1) * row_bytes / med / 1e9
        print("  mix kernel, all instances, %-13s median %9.3f ms  fastest %9.3f   %6.2f TB/s = %4.1f%% of the copy rate (bytes / 6.29 TB/s = %.3f ms); + %.1f%% on the render"
              % (label, med, best, rate / 1e3, 100 * rate * 1e9 / COPY_RATE, floor, 100 * med / t_render), flush=True)
    for mb in TILES_MB:  # one tile, mixed right after the render wrote it (what dusp_render_host_mix does per tile)
        tile = min(V, max(1, (mb << 20) // row_bytes))
        dt = torch.from_numpy(np.ascontiguousarray(params[:, :tile])).cuda()
        times = []
        for r in range(reps + 1):
            prog.render_device(n, tile, dt.data_ptr(), out.data_ptr(), s)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            ctxs["by grid"].mix(out.data_ptr(), tile, C, n, acc.data_ptr(), None, None, True, s)
            b.record(stream)
            b.synchronize()
            if r:
                times.append(a.elapsed_time(b))
        med = float(np.median(times))
        print("  mix of one %4d MiB tile after its render  %6d instances, %7.1f MB  median %9.3f ms  %6.2f TB/s" % (mb, tile, tile * row_bytes / 1e6, med, (tile + 1) * row_bytes / med / 1e12), flush=True)
    del out, acc
    torch.cuda.empty_cache()
    prog.close()
    for mb, ctx in tile_ctxs.items():  # the host call, by default tile
        p = ctx.build(uni.words)
        times = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            res = p.render_mix(n, V, params, pinned=True)
            dt_ = time.perf_counter() - t0
            del res
            if r:
                times.append(dt_ * 1e3)
        # (0: the library's own default — 32 instances a compute unit within 16 GiB; free memory does not bind on these cases)
        tile = min(V, max(1, (mb << 20) // row_bytes)) if mb else min(V, 32 * n_cus, max(1, (16 << 30) // row_bytes))
        print("  render_mix, host clock, %s tiles (%6d instances, %4d tiles)  median %9.2f ms  fastest %9.2f   x%.2f of the render alone"
              % ("%4d MiB" % mb if mb else " default", tile, -(-V // tile), float(np.median(times)), min(times), float(np.median(times)) / t_render), flush=True)
        p.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide every case's voice count by this (a quick look)")
    ap.add_argument("--sweep-all", action="store_true", help="the tile sweep of the host call on every case, not only a and b")
    a = ap.parse_args()
    os.environ["DUSP_WAVE_JIT"] = "2"  # wait for compiled kernels
    ctxs = {"by grid": context(), "1 float x 8": context(DUSP_MIX_WIDTH=1, DUSP_MIX_DEPTH=8), "1 float x 32": context(DUSP_MIX_WIDTH=1, DUSP_MIX_DEPTH=32),
            "4 floats x 8": context(DUSP_MIX_WIDTH=4)}
    tile_ctxs = {0: context(), **{mb: context(DUSP_MIX_TILE_MB=mb) for mb in TILES_MB}}
    for key, spec in cases(a.scale).items():
        if key in a.cases:
            run_case(key, spec, ctxs, tile_ctxs if (a.sweep_all or key in "ab") else {0: tile_ctxs[0]}, a.reps)


if __name__ == "__main__":
    main()
