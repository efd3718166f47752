'use strict'
/* Stems in the JavaScript host (dusp_amd/js): the `stems` option of renderPiece / renderScore and their Pcm / Wav forms.
 *   node check_stems.js --sampleRate=48000 surface
 *       no device: the refusal string, the names and what a call over a timeline of no samples resolves to, as one JSON line that
 *       tests/test_js_stems.py holds to Python's twin (mix.STEMS_NOT_BOOL, mix.stem_names, render.Stems)
 *   node check_stems.js --sampleRate=48000 render <spec.json>
 *       GPU: renderPiece / renderPiecePcm / renderScore with stems against the bits Python's calls wrote */
const fs = require('fs')
const lib = require('../../dusp_amd/js')
const rcd = require('../../dusp_amd/js/lib/renderChannelData')

const VOICES = { // twins of tests/score_voices.py voice and tests/test_piece_host.py saw_voice
  score: (k) => new lib.Multiply(new lib.Osc(200.5 + 31 * k), new lib.Ramp(700, 1, 0).trigger()),
  saw: (k) => new lib.Multiply(new lib.Filter(new lib.Osc(110 + 3.25 * k, 'saw'), 900 + 40 * k), new lib.Ramp(1000, 1, 0).trigger()),
}
const interleaved = (n) => Array.from({ length: n }, (_, k) => VOICES[k % 2 === 0 ? 'score' : 'saw'](k >> 1))

// twins of tests/master_cases.py
const echoOf = (delay) => (x) => {
  const s = new lib.Sum(x, 0)
  s.B = new lib.Multiply(new lib.Delay(s, delay, 2048), 0.5)
  return s
}
const echo = echoOf(300.25)
const clip = (x) => { const c = new lib.Clip(0.8); c.IN = new lib.Multiply(x, 1.7); return c }
const comb = (x) => { const u = new lib.CombFilter(100 / 48000, 0.6); u.IN = x; return u }

async function rejection(f) {
  try { await f() } catch (e) { return typeof e === 'string' ? e : 'not a string: ' + e }
  return null
}

async function surface() {
  const mono = () => [VOICES.score(0), VOICES.score(1), VOICES.score(2)]
  const base = { onsets: [0, 1, 2], voiceDurations: 0.01, voiceDuration: 0.01, duration: 0 }
  const calls = { renderPiece: lib.renderPiece, renderScore: lib.renderScore, renderPiecePcm: lib.renderPiecePcm, renderScorePcm: lib.renderScorePcm, renderPieceWav: lib.renderPieceWav, renderScoreWav: lib.renderScoreWav }
  const refused = {}
  for (const [name, call] of Object.entries(calls))
    refused[name] = [await rejection(() => call(mono(), Object.assign({ stems: 1, pans: [0] }, base))), await rejection(() => call(mono(), Object.assign({ stems: null }, base))),
      await rejection(() => call(mono(), Object.assign({ stems: 'mix' }, base)))]
  const withTracks = { tracks: [echo, null], trackOf: [0, 1, -1], faders: [1, 0.5], buses: [comb], trackSends: [[1, 0]] }
  const empty = await lib.renderScore(mono(), Object.assign({ stems: true }, base, withTracks))
  const pcm = await lib.renderPiecePcm(mono(), Object.assign({ stems: true, bitDepth: 24, normalise: 2 }, base))
  const off = await lib.renderScore(mono(), Object.assign({ stems: false }, base, withTracks))
  const report = {
    refused,
    names: [rcd.stemNames(0, 0), rcd.stemNames(2, 1), rcd.stemNames(8, 4)],
    empty: { names: empty.names, tracks: empty.tracks.length, buses: empty.buses.length, mix: empty.mix.length, sampleRate: empty.mix.sampleRate, peaks: Object.keys(empty.peaks), peak: empty.peak, gain: empty.gain === undefined },
    pcm: { names: pcm.names, tracks: pcm.tracks.length, buses: pcm.buses.length, bytes: pcm.mix.data.length, bitDepth: pcm.direct.bitDepth, gain: pcm.gain },
    off: Array.isArray(off) && off.names === undefined && off.length === 0,
    commonPeak: [rcd.commonPeak([0.5, 2, 1]), rcd.commonPeak([]), Number.isNaN(rcd.commonPeak([1, NaN, Infinity]))],
  }
  console.log(JSON.stringify(report))
}

function sameBits(a, b) {
  if (a.length !== b.length) return false
  const x = new Uint32Array(a.buffer, a.byteOffset, a.length), y = new Uint32Array(b.buffer, b.byteOffset, b.length)
  for (let t = 0; t < x.length; t++) if (x[t] !== y[t]) return false
  return true
}

function rawFile(path) {
  const raw = fs.readFileSync(path)
  return raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length)
}

/* a call's stems against the planar f32 [signals][channels][samples] and the peaks [signals] Python wrote */
function held(got, names, want, wantPeaks, channels) {
  if (JSON.stringify(got.names) !== JSON.stringify(names)) return false
  const signals = [got.direct].concat(got.tracks, got.buses, [got.mix]), n = want.length / names.length / channels
  return signals.length === names.length && signals.every((signal, s) => signal.length === channels && signal.every((ch, c) => sameBits(ch, want.subarray((s * channels + c) * n, (s * channels + c + 1) * n)))) &&
    sameBits(Float32Array.from(names, (name) => got.peaks[name]), wantPeaks) && sameBits(Float32Array.of(got.peak), Float32Array.of(wantPeaks.reduce((a, b) => Math.max(a, b), 0)))
}

async function render(specPath) {
  const spec = JSON.parse(fs.readFileSync(specPath, 'utf8'))
  const f32 = (tag) => new Float32Array(rawFile(specPath.replace(/\.json$/, tag + '.f32')))
  const report = { failed: [], checked: 0 }
  const note = (name, ok) => { report.checked++; if (!ok) report.failed.push(name) }
  const opts = (tileBytes, extra) => Object.assign({ onsets: spec.onsets, gains: spec.gains, voiceDurations: spec.voiceDurations, duration: spec.duration, tileBytes, stems: true }, extra)
  const tracked = { tracks: [clip, null, echo], trackOf: spec.trackOf3, faders: spec.faders3, buses: [echo, comb], trackSends: spec.trackSends }
  for (const tileBytes of [0, 9000]) {
    const got = await lib.renderPiece(interleaved(spec.n), opts(tileBytes, tracked))
    note('tracks and buses, tileBytes ' + tileBytes, held(got, ['direct', 'track0', 'track1', 'track2', 'bus0', 'bus1', 'mix'], f32('.full'), f32('.full.peaks'), 1))
  }
  const without = await lib.renderPiece(interleaved(spec.n), opts(0, Object.assign({}, tracked, { stems: false })))
  const full = f32('.full')
  note('the mix is the call without stems', without.length === 1 && sameBits(without[0], full.subarray(full.length - without[0].length)))
  const mastered = await lib.renderPiece(interleaved(spec.n), opts(0, Object.assign({ master: comb }, tracked)))
  note('a master behind them', held(mastered, ['direct', 'track0', 'track1', 'track2', 'bus0', 'bus1', 'mix'], f32('.master'), f32('.master.peaks'), 1))
  const sent = await lib.renderPiece(Array.from({ length: spec.n }, (_, k) => VOICES.score(k)), opts(0, { voiceDurations: spec.voiceDurations[0], pans: spec.pans, buses: [echo], sends: [spec.sends] }))
  note('per-note sends with pans', held(sent, ['direct', 'bus0', 'mix'], f32('.sends'), f32('.sends.peaks'), 2))
  const plain = await lib.renderPiece(interleaved(spec.n), opts(0))
  note('neither tracks nor buses', held(plain, ['direct', 'mix'], f32('.plain'), f32('.plain.peaks'), 1))
  const score = await lib.renderScore(Array.from({ length: spec.n }, (_, k) => VOICES.score(k)), { onsets: spec.onsets, gains: spec.gains, voiceDuration: spec.voiceDurations[0], duration: spec.duration,
    stems: true, tracks: [echo, comb], trackOf: spec.trackOf2, faders: spec.faders2 })
  note('renderScore with stems', held(score, ['direct', 'track0', 'track1', 'mix'], f32('.score'), f32('.score.peaks'), 1))
  // frames: the loud case's s16 under the common gain, and the files over them
  const loud = () => Array.from({ length: spec.loudOnsets.length }, (_, k) => VOICES.score(k >> 1))
  const loudOpts = { onsets: spec.loudOnsets, gains: spec.loudGains, voiceDurations: spec.voiceDurations[0], duration: spec.duration, tracks: [null, null], trackOf: spec.loudTrackOf, faders: [1, -1], stems: true,
    bitDepth: 16, normalise: 2 }
  const pcm = await lib.renderPiecePcm(loud(), loudOpts)
  const wantFrames = Buffer.from(rawFile(specPath.replace(/\.json$/, '.loud.s16'))), each = wantFrames.length / 4
  const frames = [pcm.direct].concat(pcm.tracks, pcm.buses, [pcm.mix])
  note('s16 frames under one gain', frames.length === 4 && frames.every((one, s) => one.bitDepth === 16 && one.numberOfChannels === 1 && one.data.equals(wantFrames.subarray(s * each, (s + 1) * each))) &&
    sameBits(Float32Array.from(pcm.names, (name) => pcm.peaks[name]), f32('.loud.peaks')) && pcm.gain === spec.loudGain && pcm.peaks.track1 > pcm.peaks.mix * 20)
  const files = await lib.renderPieceWav(loud(), loudOpts)
  note('a file a signal', files.names.length === 4 && files.mix.length === 44 + each && files.mix.subarray(44).equals(pcm.mix.data) && files.tracks[1].subarray(44).equals(pcm.tracks[1].data))
  console.log(JSON.stringify(report))
}

const mode = process.argv.find((a) => a === 'surface' || a === 'render')
const run = mode === 'surface' ? surface() : render(process.argv[process.argv.indexOf('render') + 1])
run.catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack ? e.stack : e) })); process.exit(1) })
