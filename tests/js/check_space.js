'use strict'
/* The `places` option of the JavaScript host (dusp_amd/js): mono voices of a score or piece placed in a space, every speaker a channel.
 *   node check_space.js --sampleRate=48000 refusals
 *       no device: the refusal strings of renderPiece / renderScore and their Pcm / Wav forms with places, and spaceTaps, as one JSON
 *       line that tests/test_space_host.py holds to Python's twin
 *   node check_space.js --sampleRate=48000 render <spec.json>
 *       GPU: renderPiece / renderPiecePcm / renderScore with places of the list the spec describes against the contract at the gains
 *       spaceTaps returned (spec.f32, which Python made from them), against Python's render_piece, whose gains the test has found equal,
 *       and against the oracle's channel-by-channel render (spec.golden), whatever tileBytes */
const fs = require('fs')
const lib = require('../../dusp_amd/js')

const VOICES = { // twins of tests/score_voices.py voice, tests/test_piece_host.py saw_voice and tests/mix_voices.py voice
  score: (k) => new lib.Multiply(new lib.Osc(200.5 + 31 * k), new lib.Ramp(700, 1, 0).trigger()),
  saw: (k) => new lib.Multiply(new lib.Filter(new lib.Osc(110 + 3.25 * k, 'saw'), 900 + 40 * k), new lib.Ramp(1000, 1, 0).trigger()),
  filtered_saw: (k) => new lib.Filter(new lib.Osc(110 + 3.25 * k, 'saw'), 900 + 40 * k),
  pan: (k) => new lib.Pan(new lib.Osc(180 + 2.5 * k), -0.9 + 0.03 * k),
}
const interleaved = (n) => Array.from({ length: n }, (_, k) => VOICES[k % 2 === 0 ? 'score' : 'saw'](k >> 1))

async function rejection(f) {
  try { await f() } catch (e) { return typeof e === 'string' ? e : 'not a string: ' + e }
  return null
}

async function refusals() {
  const mono = () => [VOICES.score(0), VOICES.score(1), VOICES.score(2)]
  const two = () => [VOICES.score(0), VOICES.filtered_saw(0), VOICES.score(1)]
  const stereo = () => [VOICES.pan(0), VOICES.pan(1), VOICES.pan(2)]
  const native = require('../../dusp_amd/js/lib/native')()
  const at = [[0, 0], [1, 1], [2, 0.5]]
  const piece = { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0.05 }, score = { onsets: [0, 1, 2], voiceDuration: 0.01, duration: 0.05 }
  const taps = lib.spaceTaps([[0, 0], [1, 2], [-2.5, 0.75], [1, 0]], { sampleRate: 48000 })
  const taps3 = lib.spaceTaps([[0, 0, 1], [3, -1, 2]], { speakers: [[-1, 0, 0], [1, 0, 0], [0, 2, 1]], decibelsPerMetre: -6, sampleDelayPerMetre: 77.5 })
  const report = {
    refusals: {
      shape: await rejection(() => lib.renderPiece(mono(), Object.assign({ places: [[0, 0], [1, 1]] }, piece))),
      shapeScore: await rejection(() => lib.renderScore(mono(), Object.assign({ places: [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]] }, score))),
      finite: await rejection(() => lib.renderPiece(mono(), Object.assign({ places: [[0, 0], [1, 1], [NaN, 0]] }, piece))),
      finitePcm: await rejection(() => lib.renderScorePcm(mono(), Object.assign({ places: [[0, 0], [1, 1], [0, Infinity]] }, score))),
      finiteWav: await rejection(() => lib.renderPieceWav(mono(), Object.assign({ places: [[0, 0], [1, 1], [0, -Infinity]] }, piece))),
      speakerFinite: await rejection(() => lib.renderPiece(mono(), Object.assign({ places: at, speakers: [[0, 0], [NaN, 1]] }, piece))),
      coordinates: await rejection(() => lib.renderPiecePcm(mono(), Object.assign({ places: at, speakers: [[0, 0, 0]] }, piece))),
      speakerCount: await rejection(() => lib.renderScoreWav(mono(), Object.assign({ places: at, speakers: Array.from({ length: 9 }, (_, k) => [0, k]) }, score))),
      pans: await rejection(() => lib.renderPiece(mono(), Object.assign({ places: at, pans: [0, 0, 0] }, piece))),
      fracs: await rejection(() => lib.renderScore(mono(), Object.assign({ places: at, fracs: [0, 0, 0] }, score))),
      mono: await rejection(() => lib.renderPiece(stereo(), Object.assign({ places: at }, piece))),
      onePart: await rejection(() => lib.renderScore(two(), Object.assign({ places: at }, score))),
      tooFar: await rejection(() => lib.renderPiece(mono(), Object.assign({ places: [[0, 0], [3e5, 0], [0, 0]], speakers: [[0, 0]] }, piece))),
    },
    addonCall: typeof native.renderPieceSpace === 'function',
    taps: { nSpeakers: taps.nSpeakers, delays: Array.from(taps.delays), gains: Array.from(taps.gains) },
    taps3: { nSpeakers: taps3.nSpeakers, delays: Array.from(taps3.delays), gains: Array.from(taps3.gains) },
  }
  console.log(JSON.stringify(report))
}

function sameBits(a, b) {
  if (a.length !== b.length) return false
  const x = new Uint32Array(a.buffer, a.byteOffset, a.length), y = new Uint32Array(b.buffer, b.byteOffset, b.length)
  for (let t = 0; t < x.length; t++) if (x[t] !== y[t]) return false
  return true
}

function floatsOf(path) {
  const raw = fs.readFileSync(path)
  const copy = new Uint8Array(raw) // (a Buffer from the pool may sit at any byte offset)
  return new Float32Array(copy.buffer, 0, copy.length / 4)
}

async function render(specPath) {
  const spec = JSON.parse(fs.readFileSync(specPath, 'utf8'))
  // planar [C][nTotal] each: the contract in numpy at the gains THIS process's spaceTaps made (spec.gains), Python's render_piece, the oracle
  const want = floatsOf(specPath.replace(/\.json$/, '.f32')), python = floatsOf(specPath.replace(/\.json$/, '.python.f32')), golden = floatsOf(spec.golden)
  const nt = spec.nTotal, C = spec.speakers.length
  const report = { failed: [], checked: 0 }
  const note = (name, ok) => { report.checked++; if (!ok) report.failed.push(name) }
  const space = { places: spec.places, speakers: spec.speakers, sampleDelayPerMetre: spec.sampleDelayPerMetre }
  const opts = (tileBytes) => Object.assign({ onsets: spec.onsets, gains: spec.voiceGains, voiceDurations: spec.voiceDurations, duration: spec.duration, tileBytes }, space)
  const taps = lib.spaceTaps(spec.places, space)
  note('the files hold the timeline\'s channels', want.length === C * nt && golden.length === C * nt && python.length === C * nt)
  note('spaceTaps gives the taps the expectation was made from', taps.nSpeakers === C && spec.delays.every((x, j) => Object.is(x, taps.delays[j])) && spec.gains.every((x, j) => Object.is(x, taps.gains[j])))
  const all = (got, ref) => got.length === C && got.every((ch, c) => sameBits(ch, ref.subarray(c * nt, (c + 1) * nt)))
  for (const tileBytes of [0, 1, 20000]) {
    const got = await lib.renderPiece(interleaved(spec.n), opts(tileBytes))
    const ok = got.length === C && got.sampleRate === spec.sampleRate && got[0].length === nt
    note('renderPiece with places is the contract at spaceTaps\' gains, tileBytes ' + tileBytes, ok && all(got, want))
    note('renderPiece with places is Python\'s, tileBytes ' + tileBytes, ok && all(got, python))
    note('renderPiece with places is the oracle\'s channel-by-channel render, tileBytes ' + tileBytes, ok && all(got, golden))
  }
  const elsewhere = await lib.renderPiece(interleaved(spec.n), Object.assign(opts(0), { places: spec.places.map((p) => [p[0] + 0.01, p[1]]) }))
  note('other places are another piece', elsewhere.length === C && !sameBits(elsewhere[0], want.subarray(0, nt)))
  const f32 = await lib.renderPiecePcm(interleaved(spec.n), Object.assign(opts(0), { bitDepth: 32 }))
  const frames = new Float32Array(f32.data.buffer, f32.data.byteOffset, f32.data.length / 4)
  let framesOk = f32.numberOfChannels === C && frames.length === C * nt
  for (let t = 0; framesOk && t < nt; t++) for (let c = 0; c < C; c++) framesOk = framesOk && Object.is(frames[C * t + c], want[c * nt + t])
  note('renderPiecePcm f32 frames interleave the channels', framesOk)
  const s16 = await lib.renderPiecePcm(interleaved(spec.n), Object.assign(opts(20000), { bitDepth: 16, normalise: 2 }))
  const wavFile = await lib.renderPieceWav(interleaved(spec.n), Object.assign(opts(20000), { bitDepth: 16, normalise: 2 }))
  note('renderPieceWav is the header and renderPiecePcm', wavFile.length === 44 + s16.data.length && s16.data.length === 2 * C * nt && wavFile.subarray(44).equals(s16.data) && Math.abs(s16.peak - spec.peak) === 0)
  const five = () => Array.from({ length: 5 }, (_, k) => VOICES.score(k))
  const few = { onsets: [0, 100, 200, 300, 400], places: [[0, 0], [1, 1], [-1, 0], [2, -2], [0.5, 3]], speakers: spec.speakers, duration: spec.duration }
  const one = await lib.renderPiece(five(), Object.assign({ voiceDurations: spec.voiceDurations[0] }, few))
  const score = await lib.renderScore(five(), Object.assign({ voiceDuration: spec.voiceDurations[0] }, few))
  note('renderScore with places is renderPiece of one structure', one.length === C && score.length === C && one.every((ch, c) => sameBits(ch, score[c])))
  const scoreWav = await lib.renderScoreWav(five(), Object.assign({ voiceDuration: spec.voiceDurations[0], bitDepth: 32 }, few))
  const scorePcm = await lib.renderScorePcm(five(), Object.assign({ voiceDuration: spec.voiceDurations[0], bitDepth: 32 }, few))
  note('renderScoreWav is the header and renderScorePcm', scorePcm.numberOfChannels === C && scoreWav.subarray(scoreWav.length - scorePcm.data.length).equals(scorePcm.data))
  console.log(JSON.stringify(report))
}

const mode = process.argv.find((a) => a === 'refusals' || a === 'render')
const run = mode === 'refusals' ? refusals() : render(process.argv[process.argv.indexOf('render') + 1])
run.catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack ? e.stack : e) })); process.exit(1) })
