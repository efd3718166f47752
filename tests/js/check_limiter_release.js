'use strict'
/* The limiter's release of its own in the JavaScript host (dusp_amd/js; DESIGN.md 6.21): the `limiterRelease` option of renderPiece /
 * renderScore and their Pcm / Wav forms, and limit()'s release.
 *   node check_limiter_release.js --sampleRate=48000 surface
 *       no device: the refusal strings, the release in samples and what a call over a timeline of no samples resolves to, as one JSON line
 *       that tests/test_js_limiter_release.py holds to Python's twin (mix.LIMITER_RELEASE_*, render.Limiter)
 *   node check_limiter_release.js --sampleRate=48000 render <spec.json>
 *       GPU: the fields of renderPiecePcm / renderPieceWav with limiter: true, limiterRelease — engaged and not — and of limit() with a
 *       release as one JSON line, with a digest of every signal's frames, which the test holds to what Python's calls returned */
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
function thrown(f) {
  try { f() } catch (e) { return typeof e === 'string' ? e : 'not a string: ' + e }
  return null
}
const num = (x) => (Number.isFinite(x) ? x : String(x))
const record = (l) => ({ engaged: l.engaged, threshold: num(l.threshold), window: l.window, reduction: num(l.reduction), lufsIn: num(l.lufsIn), truePeakIn: num(l.truePeakIn), release: l.release })
const plain = (meters) => ({ names: meters.names, lufs: meters.names.map((k) => num(meters.lufs[k])), rms: meters.names.map((k) => Array.from(meters.rms[k], num)),
  truePeak: meters.names.map((k) => Array.from(meters.truePeak[k], num)) })
const digest = (buf) => crypto.createHash('sha256').update(Buffer.from(buf.buffer, buf.byteOffset, buf.byteLength)).digest('hex')
const signalsOf = (got) => got.names.map((name, s) => (s === 0 ? got.direct : s === got.names.length - 1 ? got.mix : s <= got.tracks.length ? got.tracks[s - 1] : got.buses[s - 1 - got.tracks.length]))

async function surface() {
  const mono = () => [voice(0), voice(1), voice(2)]
  const base = { onsets: [0, 1, 2], voiceDurations: 0.01, voiceDuration: 0.01, duration: 0 }
  const calls = { renderPiece: lib.renderPiece, renderScore: lib.renderScore, renderPiecePcm: lib.renderPiecePcm, renderScorePcm: lib.renderScorePcm, renderPieceWav: lib.renderPieceWav, renderScoreWav: lib.renderScoreWav }
  const planar = {}, pcm = {}
  for (const [name, call] of Object.entries(calls)) {
    if (name === 'renderPiece' || name === 'renderScore')
      planar[name] = [await rejection(() => call(mono(), Object.assign({ limiter: true, loudness: -16, limiterRelease: 0.05 }, base))), await rejection(() => call(mono(), Object.assign({ limiter: true, limiterRelease: 0.05 }, base))),
        await rejection(() => call(mono(), Object.assign({ limiterRelease: 0.05 }, base)))]
    else
      pcm[name] = [await rejection(() => call(mono(), Object.assign({ loudness: -16, limiterRelease: 0.05 }, base))), await rejection(() => call(mono(), Object.assign({ limiterRelease: 0.05 }, base))),
        await rejection(() => call(mono(), Object.assign({ limiter: true, loudness: -16, limiterRelease: 0 }, base))), await rejection(() => call(mono(), Object.assign({ limiter: true, loudness: -16, limiterRelease: NaN }, base))),
        await rejection(() => call(mono(), Object.assign({ limiter: true, loudness: -16, limiterRelease: '50ms' }, base))), await rejection(() => call(mono(), Object.assign({ limiter: true, loudness: -16, limiterRelease: true }, base))),
        await rejection(() => call(mono(), Object.assign({ limiter: true, loudness: -16, limiterRelease: 1000 }, base))), await rejection(() => call(mono(), Object.assign({ limiter: true, loudness: -16, limiterRelease: 1e300 }, base))),
        await rejection(() => call(mono(), Object.assign({ limiter: true, loudness: -16, limiterWindow: 1, limiterRelease: 1000 }, base))), await rejection(() => call(mono(), Object.assign({ limiter: true, limiterRelease: 0.05 }, base)))]
  }
  const one = await lib.renderPiecePcm(mono(), Object.assign({ loudness: -16, bitDepth: 24, limiter: true, limiterRelease: 0.05 }, base))
  const none = await lib.renderScorePcm(mono(), Object.assign({ loudness: -16, limiter: true }, base))
  const x = [new Float32Array(4)]
  console.log(JSON.stringify({
    planar, pcm,
    one: { keys: Object.keys(one).sort(), gain: one.gain, limiter: record(one.limiter) },
    none: record(none.limiter),
    releases: [[0.05, 48000], [0.5, 44100], [1e-9, 8000], [4194304 / 48000, 48000], [0.0025, 1000], [0.0035, 1000], [1, 8000]].map(([r, rate]) => rcd.checkLimiterRelease(r, true, rate)),
    absent: [rcd.checkLimiterRelease(undefined, false, 48000), rcd.checkLimiterRelease(null, true, 48000)],
    limit: [thrown(() => lib.limit(x, 48000, 1, 40, 0)), thrown(() => lib.limit(x, 48000, 1, 40, 4194305)), thrown(() => lib.limit(x, 48000, 1, 40, 2.5)), thrown(() => lib.limit(x, 48000, 1, 40, true))],
    empty: (() => { const got = lib.limit([new Float32Array(0), new Float32Array(0)], 8000, 0.5, 40, 400); return [got.data.length, got.gain.length, got.reduction] })(),
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
  const engaged = await lib.renderPiecePcm(voices(), opts({ loudness: spec.high, truePeakMax: -1, bitDepth: 24, limiter: true, limiterRelease: 0.05 }))
  report.engaged = Object.assign(plain(engaged.meters), { gain: engaged.gain, level: engaged.level, limiter: record(engaged.limiter), frames: signalsOf(engaged).map((one) => digest(one.data)),
    peaks: engaged.names.map((k) => num(engaged.peaks[k])) })
  const idle = await lib.renderPiecePcm(voices(), opts({ loudness: spec.low, bitDepth: 16, limiter: true, limiterWindow: 0.01, limiterRelease: 0.5 }))
  report.idle = Object.assign(plain(idle.meters), { gain: idle.gain, level: idle.level, limiter: record(idle.limiter), frames: signalsOf(idle).map((one) => digest(one.data)) })
  const files = await lib.renderPieceWav(voices(), opts({ stems: false, loudness: spec.high, bitDepth: 16, limiter: true, limiterRelease: 0.2 }))
  report.files = { gain: files.gain, level: files.level, limiter: record(files.limiter), file: digest(files.mix) }
  const n = host.length / 6
  const signals = [0, 1, 2].map((s) => [host.subarray((2 * s) * n, (2 * s + 1) * n), host.subarray((2 * s + 1) * n, (2 * s + 2) * n)])
  const many = lib.limit(signals, spec.hostRate, spec.threshold, spec.window, spec.release)
  report.host = { data: digest(Float32Array.from([].concat(...many.data.map((sig) => [].concat(...sig.map((ch) => Array.from(ch))))))), gain: digest(many.gain), reduction: many.reduction }
  const without = lib.limit(signals, spec.hostRate, spec.threshold, spec.window)
  report.hostPlain = { gain: digest(without.gain), reduction: without.reduction }
  console.log(JSON.stringify(report))
}

const mode = process.argv.find((a) => a === 'surface' || a === 'render')
const run = mode === 'surface' ? surface() : render(process.argv[process.argv.indexOf('render') + 1])
run.catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack ? e.stack : e) })); process.exit(1) })
