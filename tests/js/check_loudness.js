'use strict'
/* Loudness delivery in the JavaScript host (dusp_amd/js): the `truePeak`, `loudness` and `truePeakMax` options of renderPiece / renderScore
 * and their Pcm / Wav forms, and truePeak().
 *   node check_loudness.js --sampleRate=48000 surface
 *       no device: the refusal strings and what a call over a timeline of no samples resolves to, as one JSON line that
 *       tests/test_js_loudness.py holds to Python's twin (mix.TRUE_PEAK_NOT_BOOL, mix.LOUDNESS_*, render.Meters)
 *   node check_loudness.js --sampleRate=48000 render <spec.json>
 *       GPU: the doubles of renderPiece with truePeak, of renderPiecePcm / renderPieceWav with loudness and of truePeak() as one JSON
 *       line, with a digest of every signal's frames, which the test holds to what Python's calls returned: the same library made both */
const crypto = require('crypto')
const fs = require('fs')
const lib = require('../../dusp_amd/js')
const rcd = require('../../dusp_amd/js/lib/renderChannelData')

const voice = (k) => new lib.Multiply(new lib.Osc(200.5 + 31 * k), new lib.Ramp(700, 1, 0).trigger()) // twin of tests/score_voices.py voice
const clip = (x) => { const c = new lib.Clip(0.8); c.IN = new lib.Multiply(x, 1.7); return c }
const comb = (x) => { const u = new lib.CombFilter(100 / 48000, 0.6); u.IN = x; return u }

async function rejection(f) {
  try { await f() } catch (e) { return typeof e === 'string' ? e : 'not a string: ' + e }
  return null
}
const num = (x) => (Number.isFinite(x) ? x : String(x))
const plain = (meters) => ({ names: meters.names, lufs: meters.names.map((k) => num(meters.lufs[k])), rms: meters.names.map((k) => Array.from(meters.rms[k], num)),
  truePeak: meters.names.map((k) => Array.from(meters.truePeak[k], num)) })
const digest = (buf) => crypto.createHash('sha256').update(Buffer.from(buf.buffer, buf.byteOffset, buf.byteLength)).digest('hex')
const signalsOf = (got) => got.names.map((name, s) => (s === 0 ? got.direct : s === got.names.length - 1 ? got.mix : s <= got.tracks.length ? got.tracks[s - 1] : got.buses[s - 1 - got.tracks.length]))

async function surface() {
  const mono = () => [voice(0), voice(1), voice(2)]
  const base = { onsets: [0, 1, 2], voiceDurations: 0.01, voiceDuration: 0.01, duration: 0 }
  const calls = { renderPiece: lib.renderPiece, renderScore: lib.renderScore, renderPiecePcm: lib.renderPiecePcm, renderScorePcm: lib.renderScorePcm, renderPieceWav: lib.renderPieceWav, renderScoreWav: lib.renderScoreWav }
  const notBool = {}, planar = {}, pcm = {}
  for (const [name, call] of Object.entries(calls)) {
    notBool[name] = [await rejection(() => call(mono(), Object.assign({ truePeak: 1, pans: [0] }, base))), await rejection(() => call(mono(), Object.assign({ truePeak: 'dBTP' }, base))),
      await rejection(() => call(mono(), Object.assign({ truePeak: 1, meters: 1 }, base)))]
    if (name === 'renderPiece' || name === 'renderScore') planar[name] = await rejection(() => call(mono(), Object.assign({ loudness: -16 }, base)))
    else
      pcm[name] = [await rejection(() => call(mono(), Object.assign({ loudness: '-16' }, base))), await rejection(() => call(mono(), Object.assign({ loudness: NaN }, base))),
        await rejection(() => call(mono(), Object.assign({ loudness: -16, truePeakMax: 0.5 }, base))), await rejection(() => call(mono(), Object.assign({ loudness: -16, truePeakMax: NaN }, base))),
        await rejection(() => call(mono(), Object.assign({ loudness: -16, normalise: 2 }, base)))]
  }
  const withTracks = { tracks: [clip, null], trackOf: [0, 1, -1], faders: [1, 0.5], buses: [comb], trackSends: [[1, 0]] }
  const empty = await lib.renderScore(mono(), Object.assign({ stems: true, truePeak: true }, base, withTracks))
  const one = await lib.renderPiecePcm(mono(), Object.assign({ loudness: -16, bitDepth: 24 }, base))
  const stems = await lib.renderPiecePcm(mono(), Object.assign({ stems: true, loudness: -23, truePeakMax: -2 }, base, withTracks))
  const off = await lib.renderPiecePcm(mono(), Object.assign({ meters: true, bitDepth: 24, normalise: 2 }, base))
  console.log(JSON.stringify({
    notBool, planar, pcm,
    empty: Object.assign(plain(empty.meters), { stems: empty.names, level: empty.level === undefined }),
    one: Object.assign(plain(one.meters), { keys: Object.keys(one).sort(), gain: one.gain, level: one.level, bytes: one.mix.data.length }),
    stems: { names: stems.names, gain: stems.gain, level: stems.level, bytes: stems.mix.data.length, meters: stems.meters.names },
    off: off.gain === undefined && off.meters.truePeak === undefined,
    none: rcd.truePeak([new Float32Array(0), new Float32Array(0)], 8000).map((a) => Array.from(a)),
  }))
}

async function render(specPath) {
  const spec = JSON.parse(fs.readFileSync(specPath, 'utf8'))
  const raw = fs.readFileSync(specPath.replace(/\.json$/, '.host.f32'))
  const host = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length))
  const voices = () => Array.from({ length: spec.n }, (_, k) => voice(k))
  const opts = (extra) => Object.assign({ onsets: spec.onsets, gains: spec.gains, voiceDurations: spec.voiceDuration, duration: spec.duration, pans: spec.pans, stems: true,
    tracks: [clip, null], trackOf: spec.trackOf, faders: spec.faders, buses: [comb], trackSends: spec.trackSends }, extra)
  const report = {}
  const planar = await lib.renderPiece(voices(), opts({ truePeak: true }))
  report.planar = Object.assign(plain(planar.meters), { stems: planar.names, level: planar.level === undefined })
  const pcm = await lib.renderPiecePcm(voices(), opts({ loudness: -23, bitDepth: 16 }))
  report.pcm = Object.assign(plain(pcm.meters), { gain: pcm.gain, level: pcm.level, frames: signalsOf(pcm).map((one) => digest(one.data)), peaks: pcm.names.map((k) => num(pcm.peaks[k])) })
  const limited = await lib.renderPiecePcm(voices(), opts({ loudness: 0, truePeakMax: -1, bitDepth: 24 }))
  report.limited = { gain: limited.gain, level: limited.level, frames: signalsOf(limited).map((one) => digest(one.data)) }
  const lone = await lib.renderPiecePcm(voices(), opts({ stems: false, loudness: -16, truePeakMax: -2, bitDepth: 24 }))
  report.lone = Object.assign(plain(lone.meters), { keys: Object.keys(lone).sort(), gain: lone.gain, level: lone.level, frames: digest(lone.mix.data), peak: num(lone.mix.peak) })
  const files = await lib.renderPieceWav(voices(), opts({ loudness: -23, bitDepth: 16 }))
  report.files = { gain: files.gain, level: files.level, files: signalsOf(files).map((one) => digest(one)) }
  const n = host.length / 6
  const signals = [0, 1, 2].map((s) => [host.subarray((2 * s) * n, (2 * s + 1) * n), host.subarray((2 * s + 1) * n, (2 * s + 2) * n)])
  report.host = lib.truePeak(signals, spec.hostRate).map((a) => Array.from(a, num))
  report.hostOne = lib.truePeak(signals[0], spec.hostRate).map((a) => Array.from(a, num))
  console.log(JSON.stringify(report))
}

const mode = process.argv.find((a) => a === 'surface' || a === 'render')
const run = mode === 'surface' ? surface() : render(process.argv[process.argv.indexOf('render') + 1])
run.catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack ? e.stack : e) })); process.exit(1) })
