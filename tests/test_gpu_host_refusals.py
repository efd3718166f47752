"""The refusals of the Python host that need a live program, by exception type and full message (tests/test_host_refusals.py holds
those that need no device): Program.render, render_pcm, render_mix and render_score, and Context.render_score_parts.  Nothing is
rendered: every call is refused on the host before the library is entered."""
import numpy as np
import pytest

import dusp_amd as d
from dusp_amd import descriptor, render

pytestmark = pytest.mark.gpu

N, NS = 2, 64  # instances, samples
PARAMS = "params must have shape (n_params=%d, n_instances=2)"
INPUTS = "inputs must have shape (n_inputs=1, n_instances=1, n_samples=64)"
FORMAT = 'dusp-hip: format must be "s16", "s24" or "f32", not %s'
NORMALISE = "dusp-hip: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale), not %s"
TILE = "dusp-hip: tile_instances must be 0 (the default tile) or at least 1"
GAINS = "dusp-hip: gains must have shape (n_instances=2,)"
IN_SAMPLES = "dusp-hip: %s are in samples, whole numbers: a fraction (or what is no number) is refused"


def test_a_live_program_refuses_by_todays_strings():
    d.configure(48000)
    ctx = render.context(48000)
    uni = descriptor.unify([descriptor.extract(d.Osc(110 + 3.25 * k, "saw")) for k in range(N)])
    fed = descriptor.extract(d.Multiply(d.HostSource(np.zeros(NS, dtype=np.float32)), 2))
    saw, src = ctx.build(uni.words), ctx.build(fed.words)
    try:
        assert saw.n_params >= 1 and saw.n_inputs == 0 and src.n_inputs == 1 and src.n_params == 0 and uni.params.shape == (saw.n_params, N)
        p, short, x = uni.params, uni.params[:, :1], np.zeros((1, 1, NS), dtype=np.float32)
        params = PARAMS % saw.n_params
        part = (saw, NS, N, p)
        table = [  # (call, message); where two arguments are wrong the message names the one found first
            (lambda: saw.render(NS, N), params),
            (lambda: saw.render(NS, N, short), params),
            (lambda: saw.render(NS, N, np.zeros((saw.n_params + 1, N)), interleaved=True), params),
            (lambda: src.render(NS, 1), INPUTS),
            (lambda: src.render(NS, 1, inputs=x[:, :, :63]), INPUTS),
            (lambda: saw.render_pcm(NS, N, short), params),
            (lambda: saw.render_pcm(NS, N, p, format="s8"), FORMAT % "'s8'"),
            (lambda: saw.render_pcm(NS, N, p, format=4), FORMAT % "4"),
            (lambda: saw.render_pcm(NS, N, p, normalise=3), NORMALISE % "3"),
            (lambda: saw.render_pcm(NS, N, short, format="u8", normalise=3), FORMAT % "'u8'"),
            (lambda: saw.render_pcm(NS, N, short, normalise=-1), NORMALISE % "-1"),
            (lambda: src.render_pcm(NS, 1, inputs=x[0]), INPUTS),
            (lambda: saw.render_mix(NS, N, short), params),
            (lambda: saw.render_mix(NS, N, p, gains=[1]), GAINS),
            (lambda: saw.render_mix(NS, N, p, tile_instances=-1), TILE),
            (lambda: saw.render_mix(NS, N, p, format="s12"), FORMAT % "'s12'"),
            (lambda: saw.render_mix(NS, N, p, format=0), FORMAT % "0"),
            (lambda: saw.render_mix(NS, N, p, format="s16", normalise=0.5), NORMALISE % "0.5"),
            (lambda: saw.render_mix(NS, N, short, gains=[1], tile_instances=-1, format="s8"), params),
            (lambda: saw.render_mix(NS, N, p, gains=[1], tile_instances=-1, format="s8"), GAINS),
            (lambda: saw.render_mix(NS, N, p, tile_instances=-1, format="s8", normalise=3), TILE),
            (lambda: saw.render_mix(NS, N, p, format="s8", normalise=3), FORMAT % "'s8'"),
            (lambda: saw.render_score(NS, 2 * NS, N, [0]), "dusp-hip: onsets must have shape (n_instances=2,)"),
            (lambda: saw.render_score(NS, 2 * NS, N, [0, 0.5]), IN_SAMPLES % "onsets"),
            (lambda: saw.render_score(NS, 2 * NS, N, [0, 1], lengths=[64, 63.5], params=p), IN_SAMPLES % "lengths"),
            (lambda: saw.render_score(NS, 2 * NS, N, [0, 1], params=short), params),
            (lambda: saw.render_score(NS, 2 * NS, N, [0, 1], params=p, gains=[1, 2, 3]), GAINS),
            (lambda: saw.render_score(NS, 2 * NS, N, [0, 1], params=p, tile_instances=-2), TILE),
            (lambda: saw.render_score(NS, 2 * NS, N, [0, 1], params=p, format="pcm"), FORMAT % "'pcm'"),
            (lambda: saw.render_score(NS, 2 * NS, N, [0, 1], params=p, format="s24", normalise=9), NORMALISE % "9"),
            (lambda: saw.render_score(NS, 2 * NS, N, [0.5, 1], lengths=[1], params=short), IN_SAMPLES % "onsets"),
            (lambda: saw.render_score(NS, 2 * NS, N, [0, 1], lengths=[1], params=short), "dusp-hip: lengths must have shape (n_instances=2,)"),
            (lambda: saw.render_score(NS, 2 * NS, N, [0, 1], params=short, gains=[1], tile_instances=-1), params),
            (lambda: saw.render_score(NS, 2 * NS, N, [0, 1], params=p, gains=[1], tile_instances=-1, format="s8"), GAINS),
            (lambda: saw.render_score(NS, 2 * NS, N, [0, 1], params=p, tile_instances=-1, format="s8"), TILE),
            (lambda: ctx.render_score_parts([], [], [], 2 * NS), "dusp-hip: a piece has at least one part"),
            (lambda: ctx.render_score_parts([part], [0, 1], [0, 1], 2 * NS), "dusp-hip: part_of names a part, 0 .. 0, for each voice"),
            (lambda: ctx.render_score_parts([part], [0, -1], [0, 1], 2 * NS), "dusp-hip: part_of names a part, 0 .. 0, for each voice"),
            (lambda: ctx.render_score_parts([part], [0.0, 0.0], [0, 1], 2 * NS), "dusp-hip: part_of names a part, 0 .. 0, for each voice"),
            (lambda: ctx.render_score_parts([part], [0, 0], [0], 2 * NS), "dusp-hip: onsets must have shape (n_instances=2,)"),
            (lambda: ctx.render_score_parts([part], [0, 0], [0, 1], 2 * NS, lengths=[0.5, 1]), IN_SAMPLES % "lengths"),
            (lambda: ctx.render_score_parts([part], [0, 0], [0, 1], 2 * NS, gains=[1]), "dusp-hip: gains must have shape (voices=2,)"),
            (lambda: ctx.render_score_parts([part], [0, 0], [0, 1], 2 * NS, tile_bytes=-1), "dusp-hip: tile_bytes must be 0 (the default tile) or a number of bytes"),
            (lambda: ctx.render_score_parts([part, (saw, NS, N, short)], [0, 0], [0, 1], 2 * NS), "dusp-hip: the params of part 1 must have shape (n_params=%d, n_instances=2)" % saw.n_params),
            (lambda: ctx.render_score_parts([part], [0, 0], [0, 1], 2 * NS, fracs=[0, 1]), "dusp-hip: the fraction of voice 1 is outside [0, 1)"),
            (lambda: ctx.render_score_parts([part], [0, 0], [0, 1], 2 * NS, pans=[0]), "dusp-hip: pans must have shape (voices=2,)"),
            (lambda: ctx.render_score_parts([part], [0, 0], [0, 1], 2 * NS, format="s8"), FORMAT % "'s8'"),
            (lambda: ctx.render_score_parts([part], [0, 0], [0, 1], 2 * NS, format="f32", normalise=3), NORMALISE % "3"),
            (lambda: ctx.render_score_parts([], [0, 9], [0.5], 2 * NS, tile_bytes=-1), "dusp-hip: a piece has at least one part"),
            (lambda: ctx.render_score_parts([part], [0, 9], [0.5], 2 * NS, tile_bytes=-1), "dusp-hip: part_of names a part, 0 .. 0, for each voice"),
            (lambda: ctx.render_score_parts([part], [0, 0], [0.5, 1], 2 * NS, gains=[1], tile_bytes=-1), IN_SAMPLES % "onsets"),
            (lambda: ctx.render_score_parts([part], [0, 0], [0, 1], 2 * NS, gains=[1], tile_bytes=-1), "dusp-hip: gains must have shape (voices=2,)"),
            (lambda: ctx.render_score_parts([(saw, NS, N, short)], [0, 0], [0, 1], 2 * NS, tile_bytes=-1), "dusp-hip: tile_bytes must be 0 (the default tile) or a number of bytes"),
            (lambda: ctx.render_score_parts([(saw, NS, N, short)], [0, 0], [0, 1], 2 * NS, fracs=[2, 2], pans=[0], format="s8"), "dusp-hip: the params of part 0 must have shape (n_params=%d, n_instances=2)" % saw.n_params),
            (lambda: ctx.render_score_parts([part], [0, 0], [0, 1], 2 * NS, fracs=[2, 2], pans=[0], format="s8"), "dusp-hip: the fraction of voice 0 is outside [0, 1)"),
            (lambda: ctx.render_score_parts([part], [0, 0], [0, 1], 2 * NS, pans=[0], format="s8", normalise=3), "dusp-hip: pans must have shape (voices=2,)"),
        ]
        for row, (call, message) in enumerate(table):
            with pytest.raises(Exception) as e:
                call()
            assert (type(e.value), str(e.value)) == (ValueError, message), row
    finally:
        saw.close()
        src.close()
