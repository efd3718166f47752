"""The PCM sample contract and the WAV writers on the host (no GPU): dusp_amd/csrc/pcm_quant.hpp against an integer-exact
evaluation, dusp_amd/wav.py against dusp_amd/js/lib/wav.js byte for byte, both decoders, the 24-bit header, and the
argument checks of Program.render_pcm."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dusp_amd import runtime, wav

NODE = shutil.which("node")
WAV_JS = os.path.join(ROOT, "dusp_amd", "js", "lib", "wav.js")
SR = 44100


def test_the_quantiser_header_equals_the_contract_in_integers(tmp_path):
    """dusp_amd/csrc/pcm_quant.hpp (what the encode kernels compute per sample) against both multiplies as exact 128-bit products
    rounded by hand and the rounding to an integer done on the mantissa: every f32 next to a rounding boundary of s16, a stride
    of s24's, three million random values, the special values; under a handful of gains."""
    exe = str(tmp_path / "pcm_quant_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "native", "pcm_quant_check.cpp")])
    rep = json.loads(subprocess.check_output([exe]).decode().strip().splitlines()[-1])
    assert rep["cases"] > 6_000_000 and rep["bad"] == 0, rep


def vector():
    """Two channels, an odd number of frames: ordinary samples, out-of-range ones, NaN, infinities, zeros, +-1 and the
    neighbours of a few rounding boundaries."""
    rng = np.random.RandomState(24)
    x = (0.6 * rng.standard_normal((2, 1237))).astype(np.float32)
    x[0, :8] = [np.nan, np.inf, -np.inf, 1.5, -3.0, 0.0, -0.0, 1.0]
    x[1, :3] = [-1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))]
    k = 11
    for scale in (32767.0, 8388607.0):
        b = np.float32(0.5 / scale)
        for f in (b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(1))):
            x[1, k], x[1, k + 1] = f, -f
            k += 2
    return x


@pytest.fixture(scope="module")
def node_files(tmp_path_factory):
    """wav.js on the vector: the three files it writes, and what its decoder reads back from each (one node process)."""
    if NODE is None:
        pytest.fail("node is needed to compare the two WAV writers")
    tmp = tmp_path_factory.mktemp("wav")
    x = vector()
    x.tofile(str(tmp / "in.f32"))
    script = """
const fs = require('fs'), path = require('path'), { encodeWav, decodeWav } = require(process.argv[2])
const dir = process.argv[3], raw = fs.readFileSync(path.join(dir, 'in.f32'))
const all = new Float32Array(raw.buffer, raw.byteOffset, raw.length / 4), n = all.length / 2
const channelData = [all.subarray(0, n), all.subarray(n)]
channelData.sampleRate = %d
for (const bitDepth of [16, 24, 32]) {
  const file = encodeWav(channelData, { bitDepth })
  fs.writeFileSync(path.join(dir, 'js' + bitDepth + '.wav'), file)
  const back = decodeWav(file)
  fs.writeFileSync(path.join(dir, 'js' + bitDepth + '.dec'), Buffer.concat(back.channelData.map((c) => Buffer.from(c.buffer, c.byteOffset, c.byteLength))))
  const nBytes = n * 2 * bitDepth / 8, pad = nBytes & 1, enc = file.slice(file.length - nBytes - pad, file.length - pad)
  if (bitDepth !== 32 && !encodeWav({ data: enc, bitDepth, numberOfChannels: 2, sampleRate: %d }).equals(file)) throw 'encoded frames + header differ from the file'
}
""" % (SR, SR)
    (tmp / "run.js").write_text(script)
    subprocess.check_call([NODE, str(tmp / "run.js"), WAV_JS, str(tmp)])
    return tmp


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_wav_py_and_wav_js_write_the_same_file(node_files, bits):
    x = vector()
    ours = wav.encode_wav(x, SR, bits)
    theirs = (node_files / ("js%d.wav" % bits)).read_bytes()
    assert ours == theirs
    # ... and from frames that are encoded already only the header is added
    if bits != 32:
        frames, _ = wav.encode_frames(x, bits, 0)
        assert wav.encode_wav(frames, SR, bits) == theirs
    assert wav.encode_wav(np.ascontiguousarray(x.T), SR, bits, frames=True) == theirs


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_both_decoders_round_trip(node_files, bits):
    x = vector()
    back = wav.decode_wav(wav.encode_wav(x, SR, bits))
    assert (back["sampleRate"], back["numberOfChannels"], back["bitDepth"], back["format"]) == (SR, 2, bits, 3 if bits == 32 else 1)
    got = back["channelData"]
    js = np.fromfile(str(node_files / ("js%d.dec" % bits)), dtype=np.float32).reshape(2, -1)
    assert got.shape == x.shape and np.array_equal(got.view(np.uint32), js.view(np.uint32))  # the two decoders agree bit for bit
    if bits == 32:
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32))
    else:
        scale = wav.SCALE[bits]
        want = (wav.quantise(x, 1.0, bits).astype(np.float64) / scale).astype(np.float32)
        assert np.array_equal(got, want)
        ordinary = np.isfinite(x) & (np.abs(x) <= 1)
        assert np.max(np.abs(got[ordinary].astype(np.float64) - x[ordinary])) <= 0.5 / scale + 2.0 ** -24  # half a step (+ the f32 rounding of the decoder's quotient)
        # encoding what was decoded gives the file again: the integers survive
        assert wav.encode_wav(got, SR, bits) == wav.encode_wav(x, SR, bits)


def test_24_bit_header_layout():
    """tag 1, block align 3 C, 16-byte fmt chunk, no fact chunk, the pad byte after an odd data chunk, the RIFF size."""
    x = vector()[:, :1237]
    assert (x.shape[1] * 2 * 3) % 2 == 0
    mono = x[:1]  # 1237 frames x 1 channel x 3 bytes: odd
    for data, n_ch in ((x, 2), (mono, 1)):
        f = wav.encode_wav(data, SR, 24)
        n_bytes = data.shape[1] * n_ch * 3
        assert f[:4] == b"RIFF" and f[8:16] == b"WAVEfmt " and struct.unpack_from("<I", f, 4)[0] == len(f) - 8
        size, tag, ch, rate, byte_rate, align, bits = struct.unpack_from("<IHHIIHH", f, 16)
        assert (size, tag, ch, rate, byte_rate, align, bits) == (16, 1, n_ch, SR, SR * n_ch * 3, 3 * n_ch, 24)
        assert f[36:40] == b"data" and struct.unpack_from("<I", f, 40)[0] == n_bytes
        assert len(f) == 44 + n_bytes + (n_bytes & 1)
        if n_bytes & 1:
            assert f[-1] == 0
        q = wav.quantise(data.T, 1.0, 24).reshape(-1)
        body = np.frombuffer(f[44:44 + n_bytes], dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        assert np.array_equal(body[:, 0] | body[:, 1] << 8 | body[:, 2] << 16, q & 0xffffff)


def test_gain_and_peak_rules():
    f32 = np.float32
    assert wav.gain(f32(0.5), 1) == 1.0 and wav.gain(f32(1.0), 1) == 1.0 and wav.gain(f32(2.0), 1) == 0.5
    assert wav.gain(f32(0.5), 2) == 2.0 and wav.gain(f32(0.0), 2) == 1.0 and wav.gain(f32(3.0), 0) == 1.0
    assert wav.gain(f32(np.inf), 2) == 1.0 and wav.gain(f32(np.nan), 1) == 1.0
    assert wav.gain(f32(3.0), 2) == 1.0 / np.float64(f32(3.0))
    x = np.array([[0.25, -0.75], [0.5, -0.0]], dtype=np.float32)
    assert wav.peak(x) == f32(0.75) and np.isnan(wav.peak(np.array([1.0, np.nan, 9.0], dtype=np.float32)))
    # floor(a + 0.5) would round the double just below 0.5 up: the contract does not
    below_half = np.nextafter(0.5, 0.0) / 32767.0
    assert float(np.float32(below_half)) * 32767.0 < 0.5 and wav.quantise(np.float32(below_half)) == 0


class _FakeContext:
    def host_empty_bytes(self, *a, **k):
        raise AssertionError("nothing may be allocated before the arguments are checked")


def test_render_pcm_argument_errors_are_messages():
    """What Program.render_pcm refuses comes back as a `dusp-hip:` string before anything is allocated or the library is called."""
    prog = runtime.Program.__new__(runtime.Program)
    prog._h, prog.ctx, prog._L = None, _FakeContext(), None
    prog.n_out_channels, prog.n_params, prog.n_inputs = 2, 0, 0
    with pytest.raises(ValueError, match="dusp-hip: format must be"):
        prog.render_pcm(100, format="s8")
    with pytest.raises(ValueError, match="dusp-hip: format must be"):
        prog.render_pcm(100, format=7)
    with pytest.raises(ValueError, match="dusp-hip: normalise must be"):
        prog.render_pcm(100, format="s24", normalise=3)
    with pytest.raises(wav.WavError, match="dusp-hip: WAV bitDepth"):
        wav.encode_wav(vector(), SR, 8)
    with pytest.raises(wav.WavError, match="sample rate"):
        wav.encode_wav(vector(), 0, 16)
