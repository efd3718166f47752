"""Device-side PCM delivery (dusp_peak_device, dusp_encode_device, dusp_render_host_pcm): the peak search, the gain, the
quantisation and the interleave on the GPU, byte for byte against the numpy statement of the sample contract
(dusp_amd/wav.py; include/dusp_hip.h "Device-side PCM delivery").  Inputs are seeded tensors, so the kernel tests need no
render; the host-render tests compare with the contract applied to the same program's own render()."""
import functools
import hashlib

import numpy as np
import pytest

import dusp_amd as d
from conftest import Golden
from dusp_amd import descriptor, render, runtime, wav

pytestmark = pytest.mark.gpu

# odd n * C (instances start off any alignment in s16 and s24), one and several tiles with tails, more than 32 channels (the
# narrower tile), one instance long enough for several workgroups of the peak kernel
SHAPES = [(1, 1, 1), (1, 1, 255), (3, 1, 257), (2, 2, 256), (3, 3, 513), (2, 5, 1001), (1, 33, 300), (2, 64, 129), (1, 2, 70001)]
FORMATS = {"s16": 16, "s24": 24, "f32": 32}
BYTES = {"s16": 2, "s24": 3, "f32": 4}
SENTINEL, GUARD = 0xC3, 64

def _planted():
    vals = [0.0, -0.0, 1.0, -1.0, 1.5, -2.25]
    for v in (1.0, -1.0):
        vals += [np.nextafter(np.float32(v), np.float32(0)), np.nextafter(np.float32(v), np.float32(2 * v))]
    for scale in (32767.0, 8388607.0):
        for k in (0, 1, 1000):
            b = np.float32((k + 0.5) / scale)
            for f in (b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(1))):
                vals += [f, -f]
    return np.array(vals, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def batch(shape, special=None):
    """Seeded planar PCM [instances, channels, samples]: 0.7 * normal, the instances scaled from well below to above full
    scale, edge values planted in the last instance (which peaks above 1 anyway)."""
    n_inst, n_ch, n = shape
    rng = np.random.RandomState(n_inst * 100003 + n_ch * 1009 + n)
    x = (0.7 * rng.standard_normal(shape)).astype(np.float32)
    x *= np.linspace(0.15, 2.5, n_inst, dtype=np.float32)[:, None, None] if n_inst > 1 else np.float32(1)
    flat = x[-1].reshape(-1)
    vals = _planted()[:flat.size]
    flat[rng.choice(flat.size, vals.size, replace=False)] = vals
    if special == "nan_inf":  # instance 0 holds a NaN, instance 1 an infinity (and both some ordinary clipping), the rest are ordinary
        x[0].reshape(-1)[[1, x[0].size // 2]] = [np.nan, 3.0]
        x[1].reshape(-1)[[0, x[1].size - 1]] = [-np.inf, np.inf]
    elif special == "zero":
        x[1] = 0.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def expected(shape, special, fmt, normalise):
    x = batch(shape, special)
    frames = [wav.encode_frames(x[i], FORMATS[fmt], normalise)[0].tobytes() for i in range(shape[0])]
    return np.frombuffer(b"".join(frames), dtype=np.uint8)


def same_peaks(got, x):
    """bit for bit abs().max() per instance; an instance with a NaN has a NaN peak (whose payload is nobody's business)"""
    want = np.array([np.abs(xi).max() for xi in x], dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (got, want)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), (got, want)


def run_device(shape, special, fmt, normalise, misalign=0):
    import torch
    ctx = render.context(48000)
    x = batch(shape, special)
    n_inst, n_ch, n = shape
    n_bytes = n_inst * n_ch * n * BYTES[fmt]
    d_in = torch.from_numpy(np.array(x)).cuda()
    d_peaks = torch.full((n_inst + 2,), -7.5, dtype=torch.float32, device="cuda")
    d_out = torch.full((GUARD + misalign + n_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")  # exactly the output, between sentinels
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.peak(d_in.data_ptr(), n_inst, n_ch, n, d_peaks.data_ptr() + 4, stream)
    ctx.encode(d_in.data_ptr(), n_inst, n_ch, n, d_out.data_ptr() + GUARD + misalign, fmt, normalise, d_peaks.data_ptr() + 4 if normalise else None, stream)
    torch.cuda.synchronize()
    peaks, out = d_peaks.cpu().numpy(), d_out.cpu().numpy()
    assert peaks[0] == -7.5 and peaks[-1] == -7.5
    same_peaks(peaks[1:-1], x)
    assert np.array_equal(d_in.cpu().numpy().view(np.uint32), x.view(np.uint32)), "the input was written to"
    lo = GUARD + misalign
    assert (out[:lo] == SENTINEL).all() and (out[lo + n_bytes:] == SENTINEL).all(), "bytes outside the output were written"
    want = expected(shape, special, fmt, normalise)
    got = out[lo:lo + n_bytes]
    assert np.array_equal(got, want), "first differing byte %d of %d" % (int(np.argmax(got != want)), n_bytes)


@pytest.mark.parametrize("normalise", [0, 1, 2])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_encode_device_equals_the_contract(shape, fmt, normalise):
    run_device(shape, None, fmt, normalise)


@pytest.mark.parametrize("misalign", [1, 2, 6, 15])
@pytest.mark.parametrize("fmt", ["s16", "s24"])
@pytest.mark.parametrize("shape", [(3, 1, 257), (3, 3, 513), (2, 64, 129)], ids=lambda s: "x".join(map(str, s)))
def test_encode_device_into_an_unaligned_buffer(shape, fmt, misalign):
    """d_out off every boundary: whole 16-byte stores between a byte-wise head and tail, nothing outside (one channel leaves
    its direct path for the general one)."""
    run_device(shape, None, fmt, 2, misalign)


def test_f32_frames_at_a_4_byte_offset():
    run_device((3, 3, 513), None, "f32", 1, 4)
    run_device((3, 1, 257), None, "f32", 2, 12)


@pytest.mark.parametrize("normalise", [0, 1, 2])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_nan_and_infinity(fmt, normalise):
    """A NaN sample makes the instance's peak NaN, an infinite one infinite: the gain falls back to 1 and, in the integer
    formats, NaN is silence and the infinities clamp; f32 keeps them."""
    shape = (4, 2, 301)
    x = batch(shape, "nan_inf")
    assert np.isnan(wav.peak(x[0])) and np.isinf(wav.peak(x[1])) and wav.gain(wav.peak(x[0]), 2) == 1.0 and wav.gain(wav.peak(x[1]), 2) == 1.0
    if fmt == "s16":
        frames = np.frombuffer(expected(shape, "nan_inf", fmt, normalise).tobytes(), dtype="<i2").reshape(4, 301, 2)
        assert frames[0].T.reshape(-1)[1] == 0 and frames[0].T.reshape(-1)[301] == 32767          # NaN -> 0; 3.0 clamps: the gain stayed 1
        assert frames[1].T.reshape(-1)[0] == -32767 and frames[1].T.reshape(-1)[-1] == 32767
    run_device(shape, "nan_inf", fmt, normalise)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_an_all_zero_instance(fmt):
    shape = (3, 2, 300)
    assert wav.peak(batch(shape, "zero")[1]) == 0.0 and wav.gain(0.0, 2) == 1.0
    run_device(shape, "zero", fmt, 2)


def test_argument_errors_are_messages():
    import torch
    ctx = render.context(48000)
    buf = torch.zeros(1024, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    for call, needle in [
        (lambda: ctx.encode(p, 1, 65, 4, p + 2048), "1..64 channels"),
        (lambda: ctx.encode(p, 1, 0, 4, p + 2048), "1..64 channels"),
        (lambda: ctx.encode(p, 1, 2, 4, p + 2048, "s8"), "format"),
        (lambda: ctx.encode(p, 1, 2, 4, p + 2048, "s16", 3), "normalise"),
        (lambda: ctx.encode(p, 1, 2, 4, p + 2048, "s16", 2, None), "d_peaks"),
        (lambda: ctx.encode(None, 1, 2, 4, p + 2048), "NULL"),
        (lambda: ctx.encode(p, 1, 2, 4, p + 2049, "f32"), "aligned"),
        (lambda: ctx.peak(p, 1, 2, 4, None), "NULL"),
        (lambda: ctx.peak(p, 1, 100, 4, p + 2048), "1..64 channels"),
    ]:
        with pytest.raises((runtime.DuspHipError, ValueError, TypeError), match=needle):
            call()


# ---- dusp_render_host_pcm --------------------------------------------------------------------------------------------------

def contract(planar, fmt, normalise):
    """[instances, channels, samples] f32 -> (data as render_pcm shapes it, peaks)"""
    enc = [wav.encode_frames(p, FORMATS[fmt], normalise) for p in planar]
    return np.stack([e[0] for e in enc]), np.array([e[1] for e in enc], dtype=np.float32)


@pytest.mark.parametrize("engine", ["auto", "chunk", "wave"])
def test_render_pcm_two_channel_golden(engine):
    g = Golden("mult_2ch")
    prog = render.context(g.sample_rate).build(g.desc, {"auto": runtime.ENGINE_AUTO, "chunk": runtime.ENGINE_CHUNK, "wave": runtime.ENGINE_WAVE}[engine])
    assert prog.n_out_channels == 2
    planar = prog.render(g.n_samples)
    for fmt in FORMATS:
        for normalise in (0, 1, 2):
            data, peaks = prog.render_pcm(g.n_samples, format=fmt, normalise=normalise)
            want, want_peaks = contract(planar, fmt, normalise)
            assert data.dtype == want.dtype and data.shape == want.shape
            assert np.array_equal(data.view(np.uint8), want.view(np.uint8)), (fmt, normalise)
            assert np.array_equal(peaks.view(np.uint32), want_peaks.view(np.uint32))
    prog.close()


def test_render_pcm_batch_with_a_parameter_table():
    """Instances with different levels: different peaks, hence different gains."""
    d.configure(48000)
    uni = descriptor.unify([descriptor.extract(d.Multiply(d.Osc(100.5 + 37 * k), [0.2 + 0.45 * k, 0.1 + 0.3 * k])) for k in range(5)])
    assert uni.n_params >= 2
    n = 256 * 5 + 77
    prog = render.context(48000).build(uni.words)
    planar = prog.render(n, uni.n_instances, uni.params)
    peaks_f = np.abs(planar).reshape(uni.n_instances, -1).max(axis=1)
    assert peaks_f.min() < 1 < peaks_f.max()
    for fmt in FORMATS:
        for normalise in (0, 1, 2):
            data, peaks = prog.render_pcm(n, uni.n_instances, uni.params, format=fmt, normalise=normalise)
            want, want_peaks = contract(planar, fmt, normalise)
            assert np.array_equal(data.view(np.uint8), want.view(np.uint8)), (fmt, normalise)
            assert np.array_equal(peaks, want_peaks) and np.array_equal(peaks, peaks_f)
    if True:  # full scale is reached by every instance under normalise = 2
        data, _ = prog.render_pcm(n, uni.n_instances, uni.params, format="s16", normalise=2)
        assert (np.abs(data.astype(np.int32)).reshape(uni.n_instances, -1).max(axis=1) == 32767).all()
    prog.close()


def test_render_pcm_across_the_staged_download_threshold():
    """32 MiB of s16 into pageable memory goes through the staged workers (byte-counted); the same render into pinned memory is
    one DMA: the same bytes, and those of the contract."""
    g = Golden("mult_2ch")
    n = (8 << 20) + 4099  # 2 channels x 2 bytes: just above 32 MiB
    prog = render.context(g.sample_rate).build(g.desc)
    planar = prog.render(n)
    want, _ = contract(planar, "s16", 2)
    digest = hashlib.sha256(want.tobytes()).hexdigest()
    del planar
    for pinned in (False, True):
        data, peaks = prog.render_pcm(n, format="s16", normalise=2, pinned=pinned)
        assert data.nbytes >= 32 << 20
        assert hashlib.sha256(data.tobytes()).hexdigest() == digest, pinned
        del data
    prog.close()


def test_render_pcm_with_a_host_generated_stream():
    """A program with an INPUT unit (how the JS host's Noise reaches the device)."""
    d.configure(48000)
    n = 256 * 6 + 31
    noise = np.random.RandomState(11).uniform(-1, 1, n).astype(np.float32)
    ex = descriptor.extract(d.Multiply(d.HostSource(noise), [1.75, 0.5]))
    prog = render.context(48000).build(ex.words)
    assert prog.n_inputs == 1
    streams = noise[None, None, :]
    planar = prog.render(n, 1, inputs=streams)
    for fmt in FORMATS:
        for normalise in (0, 1, 2):
            data, peaks = prog.render_pcm(n, 1, format=fmt, normalise=normalise, inputs=streams)
            want, want_peaks = contract(planar, fmt, normalise)
            assert np.array_equal(data.view(np.uint8), want.view(np.uint8)), (fmt, normalise)
            assert np.array_equal(peaks, want_peaks) and peaks[0] > 1
    with pytest.raises(runtime.DuspHipError, match="input streams"):
        rc = prog._L.dusp_render_host_pcm(prog._h, 1, n, None, None, 1, 0, np.empty(2 * n, np.int16).ctypes.data, None)
        prog.ctx._check(rc)
    prog.close()


def test_render_py_surface():
    """render_pcm / render_wav: an event-free circuit is encoded on the device, one with a scheduled event arrives as f32
    segments and is encoded on the host by the same contract — the same bytes as encoding renderChannelData's result."""
    d.configure(48000)
    dur = 0.05

    def plain():
        return d.Multiply(d.Multiply(d.Osc(440), 1.5), [1.0, 0.25])

    def evented():
        gain = d.Multiply(d.Osc(440), 1.5)
        gain.schedule(0.02, lambda unit: setattr(unit, "B", 0.75))
        return d.Multiply(gain, [1.0, 0.25])

    for build in (plain, evented):
        chans = d.renderChannelData(build(), dur)
        planar = np.stack([np.asarray(c) for c in chans])
        for bits in (16, 24, 32):
            for normalise in (0, 2):
                res = render.render_pcm(build(), dur, bits, normalise)
                want, peak = wav.encode_frames(planar, bits, normalise)
                assert np.array_equal(res.data.view(np.uint8), want.view(np.uint8)), (build.__name__, bits, normalise)
                assert res.peak == peak and res.numberOfChannels == 2 and res.sampleRate == 48000 and res.bitDepth == bits
        assert render.render_wav(build(), dur, 16) == wav.encode_wav(chans, 48000, 16)
        assert render.render_wav(build(), dur, 24) == wav.encode_wav(chans, 48000, 24)
        assert render.render_wav(build(), dur, 32) == wav.encode_wav(chans, 48000, 32)
