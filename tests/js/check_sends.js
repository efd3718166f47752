'use strict'
/* Effect sends in the JavaScript host (dusp_amd/js): the `buses` and `sends` options of renderPiece / renderScore.
 *   node check_sends.js --sampleRate=48000 surface
 *       no device: the refusal strings of sends and of a bus, and checkSends' table, as one JSON line that tests/test_js_sends.py holds
 *       to Python's twin (mix.check_sends, render.master_program(bus=), mix.BUS_*, mix.SENDS_*)
 *   node check_sends.js --sampleRate=48000 render <spec.json>
 *       GPU: renderPiece / renderPiecePcm / renderScore with buses against the bits Python's render_piece wrote */
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
const scheduled = (x) => { const u = clip(x); u.schedule(0.01, () => {}); return u }

async function rejection(f) {
  try { await f() } catch (e) { return typeof e === 'string' ? e : 'not a string: ' + e }
  return null
}

async function surface() {
  const rate = lib.config.sampleRate
  const refuse = (bus, channels) => rejection(() => rcd.masterProgram(bus, channels, rate, 1))
  const mono = () => [VOICES.score(0), VOICES.score(1), VOICES.score(2)]
  const s = [0.5, 0, 1]
  const piece = (extra) => rejection(() => lib.renderPiece(mono(), Object.assign({ onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0 }, extra)))
  const report = {
    table: Array.from(rcd.checkSends([[0, 0.5, 1], [1, 2, 3]], 3, 2)),
    oneBus: Array.from(rcd.checkSends(Float32Array.of(0.25, 0.5, 1), 3, 1)),
    bus: {
      notCallable: await refuse(5, 1),
      emptyList: await refuse([], 1),
      count: await refuse([echo], 2),
      noInput: await refuse(() => VOICES.score(0), 1),
      hostSource: await refuse((x) => new lib.Sum(x, new lib.Noise()), 1),
      events: await refuse(scheduled, 1),
      channels: await refuse((x) => new lib.Pan(x, 0.25), 1),
      notIsomorphic: await refuse([echo, clip], 2),
    },
    sends: {
      withoutBuses: await piece({ sends: s }),
      withoutSends: await piece({ buses: [echo] }),
      none: await piece({ buses: [], sends: s }),
      five: await piece({ buses: [echo, echo, echo, echo, echo], sends: [s, s, s, s, s] }),
      notAList: await piece({ buses: echo, sends: s }),
      fracs: await piece({ buses: [echo], sends: s, fracs: [0, 0, 0] }),
      places: await piece({ buses: [echo], sends: s, places: [[0, 0], [1, 1], [2, 0]], speakers: [[-1, 0], [1, 0]] }),
      stereo: await piece({ buses: [echo], sends: s, stereo: true }),
      short: await piece({ buses: [echo], sends: [0.5, 1] }),
      oneRowForTwo: await piece({ buses: [echo, clip], sends: s }),
      notFinite: await piece({ buses: [echo], sends: [0.5, Infinity, 1] }),
      tooLarge: await piece({ buses: [echo, clip], sends: [s, [1, 2, 1e39]] }),
      // ... and through every call that takes the options
      score: await rejection(() => lib.renderScore(mono(), { onsets: [0, 1, 2], voiceDuration: 0.01, duration: 0, sends: s })),
      piecePcm: await rejection(() => lib.renderPiecePcm(mono(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0, sends: s })),
      scoreWav: await rejection(() => lib.renderScoreWav(mono(), { onsets: [0, 1, 2], voiceDuration: 0.01, duration: 0, sends: s })),
      badBusInACall: await piece({ buses: [echo, 5], sends: [s, s] }),
    },
    noSamples: (await lib.renderPiece(mono(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0, buses: [echo], sends: s })).length,
  }
  console.log(JSON.stringify(report))
}

function sameBits(a, b) {
  if (a.length !== b.length) return false
  const x = new Uint32Array(a.buffer, a.byteOffset, a.length), y = new Uint32Array(b.buffer, b.byteOffset, b.length)
  for (let t = 0; t < x.length; t++) if (x[t] !== y[t]) return false
  return true
}

function f32File(path) {
  const raw = fs.readFileSync(path)
  return new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length))
}

async function render(specPath) {
  const spec = JSON.parse(fs.readFileSync(specPath, 'utf8'))
  const file = (tag) => f32File(specPath.replace(/\.json$/, tag + '.f32'))
  const want = file(''), wantThree = file('.three'), wantPan = file('.pan'), wantScore = file('.score'), wantMaster = file('.master')
  const report = { failed: [], checked: 0 }
  const note = (name, ok) => { report.checked++; if (!ok) report.failed.push(name) }
  const opts = (tileBytes, extra) => Object.assign({ onsets: spec.onsets, gains: spec.gains, voiceDurations: spec.voiceDurations, duration: spec.duration, tileBytes,
    buses: [echo], sends: spec.sends[0] }, extra)
  for (const tileBytes of [0, 9000]) {
    const got = await lib.renderPiece(interleaved(spec.n), opts(tileBytes))
    note('renderPiece with an echo bus, tileBytes ' + tileBytes, got.length === 1 && got.sampleRate === spec.sampleRate && sameBits(got[0], want))
  }
  const plain = await lib.renderPiece(interleaved(spec.n), opts(0, { buses: undefined, sends: undefined }))
  note('the bus changes the piece', !sameBits(plain[0], want))
  const three = await lib.renderPiece(interleaved(spec.n), opts(0, { buses: [echo, comb, clip], sends: spec.sends }))
  note('three buses', three.length === 1 && sameBits(three[0], wantThree))
  const mastered = await lib.renderPiece(interleaved(spec.n), opts(9000, { buses: [echo, clip], sends: [spec.sends[0], spec.sends[2]], master: comb }))
  note('buses and a master', mastered.length === 1 && sameBits(mastered[0], wantMaster))
  const f32 = await lib.renderPiecePcm(interleaved(spec.n), opts(0, { bitDepth: 32 }))
  note('renderPiecePcm f32 frames', f32.numberOfChannels === 1 && sameBits(new Float32Array(f32.data.buffer, f32.data.byteOffset, f32.data.length / 4), want))
  const s16 = await lib.renderPiecePcm(interleaved(spec.n), opts(9000, { bitDepth: 16, normalise: 2 }))
  const wavFile = await lib.renderPieceWav(interleaved(spec.n), opts(9000, { bitDepth: 16, normalise: 2 }))
  note('renderPieceWav is the header and renderPiecePcm', wavFile.length === 44 + s16.data.length && wavFile.subarray(44).equals(s16.data) && Math.abs(s16.peak - spec.peak) === 0)
  // panned mono voices, a bus a channel: the send is post-pan
  const score5 = () => Array.from({ length: 5 }, (_, k) => VOICES.score(k))
  const five = { onsets: spec.fiveOnsets, gains: spec.fiveGains, duration: spec.duration }
  const pan = await lib.renderPiece(score5(), Object.assign({ voiceDurations: spec.voiceDurations[0], pans: spec.pans, buses: [[echoOf(300.25), echoOf(411.5)]], sends: [spec.fiveSends] }, five))
  note('pans, a bus a channel', pan.length === 2 && sameBits(pan[0], wantPan.subarray(0, want.length)) && sameBits(pan[1], wantPan.subarray(want.length)))
  // a score with buses goes the piece's way
  const score = await lib.renderScore(score5(), Object.assign({ voiceDuration: spec.voiceDurations[0], buses: [echo], sends: spec.fiveSends }, five))
  note('renderScore with a bus', score.length === 1 && sameBits(score[0], wantScore))
  console.log(JSON.stringify(report))
}

const mode = process.argv.find((a) => a === 'surface' || a === 'render')
const run = mode === 'surface' ? surface() : render(process.argv[process.argv.indexOf('render') + 1])
run.catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack ? e.stack : e) })); process.exit(1) })
