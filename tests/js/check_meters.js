'use strict'
/* Meters in the JavaScript host (dusp_amd/js): the `meters` option of renderPiece / renderScore and their Pcm / Wav forms, and meter().
 *   node check_meters.js --sampleRate=48000 surface
 *       no device: the refusal strings, the block count and what a call over a timeline of no samples resolves to, as one JSON line that
 *       tests/test_js_meters.py holds to Python's twin (mix.METERS_NOT_BOOL, mix.METER_RATE_LOW, mix.meter_blocks, render.Meters)
 *   node check_meters.js --sampleRate=48000 render <spec.json>
 *       GPU: the doubles of renderPiece / renderPiecePcm / renderScore with meters and of meter() as one JSON line (strings for what is
 *       not finite), which the test holds to the doubles Python's calls returned: the same library computed both */
const fs = require('fs')
const lib = require('../../dusp_amd/js')
const rcd = require('../../dusp_amd/js/lib/renderChannelData')

const VOICES = { // twins of tests/score_voices.py voice and tests/test_piece_host.py saw_voice
  score: (k) => new lib.Multiply(new lib.Osc(200.5 + 31 * k), new lib.Ramp(700, 1, 0).trigger()),
  saw: (k) => new lib.Multiply(new lib.Filter(new lib.Osc(110 + 3.25 * k, 'saw'), 900 + 40 * k), new lib.Ramp(1000, 1, 0).trigger()),
}
const interleaved = (n) => Array.from({ length: n }, (_, k) => VOICES[k % 2 === 0 ? 'score' : 'saw'](k >> 1))
const echo = (x) => {
  const s = new lib.Sum(x, 0)
  s.B = new lib.Multiply(new lib.Delay(s, 300.25, 2048), 0.5)
  return s
}
const clip = (x) => { const c = new lib.Clip(0.8); c.IN = new lib.Multiply(x, 1.7); return c }
const comb = (x) => { const u = new lib.CombFilter(100 / 48000, 0.6); u.IN = x; return u }

async function rejection(f) {
  try { await f() } catch (e) { return typeof e === 'string' ? e : 'not a string: ' + e }
  return null
}
const num = (x) => (Number.isFinite(x) ? x : String(x))
const plain = (meters) => ({ names: meters.names, hop: meters.hop, block: meters.block, lufs: meters.names.map((k) => num(meters.lufs[k])),
  rms: meters.names.map((k) => Array.from(meters.rms[k], num)), momentary: meters.names.map((k) => Array.from(meters.momentary[k], num)) })

async function surface() {
  const mono = () => [VOICES.score(0), VOICES.score(1), VOICES.score(2)]
  const base = { onsets: [0, 1, 2], voiceDurations: 0.01, voiceDuration: 0.01, duration: 0 }
  const calls = { renderPiece: lib.renderPiece, renderScore: lib.renderScore, renderPiecePcm: lib.renderPiecePcm, renderScorePcm: lib.renderScorePcm, renderPieceWav: lib.renderPieceWav, renderScoreWav: lib.renderScoreWav }
  const refused = {}
  for (const [name, call] of Object.entries(calls))
    refused[name] = [await rejection(() => call(mono(), Object.assign({ meters: 1, pans: [0] }, base))), await rejection(() => call(mono(), Object.assign({ meters: null }, base))),
      await rejection(() => call(mono(), Object.assign({ meters: 'lufs' }, base))), await rejection(() => call(mono(), Object.assign({ meters: 1, stems: 1 }, base)))]
  const withTracks = { tracks: [echo, null], trackOf: [0, 1, -1], faders: [1, 0.5], buses: [comb], trackSends: [[1, 0]] }
  const empty = await lib.renderScore(mono(), Object.assign({ stems: true, meters: true }, base, withTracks))
  const one = await lib.renderPiecePcm(mono(), Object.assign({ meters: true, bitDepth: 24, normalise: 2 }, base))
  const off = await lib.renderPiece(mono(), Object.assign({ meters: false }, base))
  const report = {
    refused,
    rateLow: [rcd.METER_RATE_LOW(7999), await rejection(async () => rcd.meter([new Float32Array(10)], 7999))],
    blocks: [[3199, 8000], [3200, 8000], [3999, 8000], [4000, 8000], [32123, 8000], [44100, 11025], [88200, 44100], [19200, 48000], [1000000, 192000]].map(([n, rate]) => rcd.meterBlocks(n, rate)),
    hops: [8000, 11025, 44100, 48000, 192000].map(rcd.meterHop),
    empty: Object.assign(plain(empty.meters), { stems: empty.names, mix: empty.mix.length }),
    one: Object.assign(plain(one.meters), { keys: Object.keys(one).sort(), bytes: one.mix.data.length, bitDepth: one.mix.bitDepth }),
    off: Array.isArray(off) && off.meters === undefined && off.length === 0,
    none: plain(rcd.meter([new Float32Array(0), new Float32Array(0)], 8000)),
  }
  console.log(JSON.stringify(report))
}

async function render(specPath) {
  const spec = JSON.parse(fs.readFileSync(specPath, 'utf8'))
  const raw = fs.readFileSync(specPath.replace(/\.json$/, '.host.f32'))
  const host = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length))
  const opts = (extra) => Object.assign({ onsets: spec.onsets, gains: spec.gains, voiceDurations: spec.voiceDurations, duration: spec.duration, meters: true }, extra)
  const tracked = { tracks: [clip, null, echo], trackOf: spec.trackOf3, faders: spec.faders3, buses: [echo, comb], trackSends: spec.trackSends }
  const report = {}
  const full = await lib.renderPiece(interleaved(spec.n), opts(Object.assign({ stems: true }, tracked)))
  report.full = plain(full.meters)
  report.fullStems = full.names
  const pcm = await lib.renderPiecePcm(interleaved(spec.n), opts(Object.assign({ stems: true, bitDepth: 16, normalise: 2 }, tracked)))
  report.pcm = plain(pcm.meters)
  const lone = await lib.renderPiece(interleaved(spec.n), opts({ master: comb }))
  report.lone = Object.assign(plain(lone.meters), { channels: lone.mix.length, samples: lone.mix[0].length })
  const without = await lib.renderPiece(interleaved(spec.n), opts({ master: comb, meters: false }))
  const a = new Uint32Array(lone.mix[0].buffer, lone.mix[0].byteOffset, lone.mix[0].length), b = new Uint32Array(without[0].buffer, without[0].byteOffset, without[0].length)
  report.loneIsTheMix = a.length === b.length && a.every((w, t) => w === b[t])
  const file = await lib.renderPieceWav(interleaved(spec.n), opts({ master: comb, bitDepth: 24, normalise: 1 }))
  report.file = Object.assign(plain(file.meters), { riff: file.mix.subarray(0, 4).toString() })
  const files = await lib.renderPieceWav(interleaved(spec.n), opts(Object.assign({ stems: true, bitDepth: 16 }, tracked)))
  report.files = Object.assign(plain(files.meters), { riff: files.mix.subarray(0, 4).toString() + files.tracks[1].subarray(0, 4).toString() })
  const score = await lib.renderScore(Array.from({ length: spec.n }, (_, k) => VOICES.score(k)), { onsets: spec.onsets, gains: spec.gains, voiceDuration: spec.voiceDurations[0], duration: spec.duration,
    meters: true, pans: spec.pans })
  report.score = plain(score.meters)
  const n = host.length / 6
  const signals = [0, 1, 2].map((s) => [host.subarray((2 * s) * n, (2 * s + 1) * n), host.subarray((2 * s + 1) * n, (2 * s + 2) * n)])
  report.host = plain(lib.meter(signals, spec.hostRate))
  report.hostOne = plain(lib.meter(signals[0], spec.hostRate))
  console.log(JSON.stringify(report))
}

const mode = process.argv.find((a) => a === 'surface' || a === 'render')
const run = mode === 'surface' ? surface() : render(process.argv[process.argv.indexOf('render') + 1])
run.catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack ? e.stack : e) })); process.exit(1) })
