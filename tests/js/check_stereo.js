'use strict'
/* The `stereo` option of the JavaScript host (dusp_amd/js): panned mono voices, plain mono voices and voices of two channels side by side
 * in a timeline of two channels.
 *   node check_stereo.js --sampleRate=48000 refusals
 *       no device: the refusal strings of renderPiece / renderScore and their Pcm / Wav forms with stereo: true, and the pans as f32
 *       with NaN for a voice that is not placed, as one JSON line that tests/test_stereo_host.py holds to Python's twin
 *   node check_stereo.js --sampleRate=48000 render <spec.json>
 *       GPU: renderPiece / renderPiecePcm / renderScore with stereo: true of the list the spec describes against the bits Python's
 *       render_piece wrote to spec.f32, against the contract (spec.contract) and against the oracle's one-circuit render (spec.golden),
 *       whatever tileBytes */
const fs = require('fs')
const lib = require('../../dusp_amd/js')
const rcd = require('../../dusp_amd/js/lib/renderChannelData')

const score = (k) => new lib.Multiply(new lib.Osc(200.5 + 31 * k), new lib.Ramp(700, 1, 0).trigger()) // twin of tests/score_voices.py voice
const VOICES = [ // twins of tests/stereo_cases.py voice: PANNED, MONO, TWO
  (k) => score(k),
  (k) => new lib.Multiply(score(k), 0.625),
  (k) => new lib.Multiply(score(k), [0.75 - 0.03125 * (k % 5), -0.5 + 0.0625 * (k % 7)]),
]
const inTurn = (n) => Array.from({ length: n }, (_, k) => VOICES[k % 3](k))
const three = (k) => new lib.Multiply(score(k), [0.5, 0.25, 0.125])

async function rejection(f) {
  try { await f() } catch (e) { return typeof e === 'string' ? e : 'not a string: ' + e }
  return null
}

async function refusals() {
  const mixed = () => [score(0), VOICES[2](1), score(2)]
  const mono = () => [score(0), score(1), score(2)]
  const wide = () => [VOICES[2](0), VOICES[2](1), VOICES[2](2)]
  const places = [[0, 1], [0, 1], [0, 1]]
  const native = require('../../dusp_amd/js/lib/native')()
  const at = { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0.05 }, atScore = { onsets: [0, 1, 2], voiceDuration: 0.01, duration: 0.05 }
  const report = {
    refusals: {
      withoutStereo: await rejection(() => lib.renderPiece(mixed(), at)),
      twoPanned: await rejection(() => lib.renderPiece(mixed(), Object.assign({ pans: [0, 0.5, null], stereo: true }, at))),
      twoPannedPcm: await rejection(() => lib.renderPiecePcm(mixed(), Object.assign({}, at, { voiceDurations: [0.01, 0.02, 0.01], pans: [null, -1, null], stereo: true }))),
      twoPannedWav: await rejection(() => lib.renderPieceWav(mixed(), Object.assign({}, at, { duration: 0, pans: [0, 0, 0], stereo: true }))),
      twoPannedScore: await rejection(() => lib.renderScore(wide(), Object.assign({ pans: [null, 0.25, null], stereo: true }, atScore))),
      channels: await rejection(() => lib.renderPiece([score(0), VOICES[2](1), three(2)], Object.assign({ stereo: true }, at))),
      shape: await rejection(() => lib.renderPiece(mixed(), Object.assign({ pans: [0, null], stereo: true }, at))),
      finite: await rejection(() => lib.renderPiece(mixed(), Object.assign({ pans: [0, null, Infinity], stereo: true }, at))),
      finiteWav: await rejection(() => lib.renderScoreWav(mono(), Object.assign({ pans: [0, null, 1e39], stereo: true }, atScore))),
      places: await rejection(() => lib.renderPiece(mixed(), Object.assign({ places, stereo: true }, at))),
      placesScorePcm: await rejection(() => lib.renderScorePcm(mono(), Object.assign({ places, stereo: true }, atScore))),
    },
    addonCall: typeof native.renderPieceStereo === 'function',
    pans: Array.from(rcd.stereoPanArrays([-1, null, NaN, 0.3, 1e-40], 5).pans, (p) => (Number.isNaN(p) ? null : p)),
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
  const want = floatsOf(specPath.replace(/\.json$/, '.f32')), golden = floatsOf(spec.golden), contract = floatsOf(spec.contract) // planar [2][nTotal] each
  const nt = spec.nTotal
  const report = { failed: [], checked: 0 }
  const note = (name, ok) => { report.checked++; if (!ok) report.failed.push(name) }
  const opts = (tileBytes) => ({ onsets: spec.onsets, gains: spec.gains, pans: spec.pans, voiceDurations: spec.voiceDuration, duration: spec.duration, tileBytes, stereo: true })
  note('the files hold two channels of the timeline', want.length === 2 * nt && golden.length === 2 * nt && contract.length === 2 * nt)
  for (const tileBytes of [0, 1, 7000]) {
    const got = await lib.renderPiece(inTurn(spec.n), opts(tileBytes))
    const ok = got.length === 2 && got.sampleRate === spec.sampleRate && got[0].length === nt
    note('renderPiece stereo is Python\'s, tileBytes ' + tileBytes, ok && sameBits(got[0], want.subarray(0, nt)) && sameBits(got[1], want.subarray(nt)))
    note('renderPiece stereo is the contract, tileBytes ' + tileBytes, ok && sameBits(got[0], contract.subarray(0, nt)) && sameBits(got[1], contract.subarray(nt)))
    note('renderPiece stereo is the oracle\'s one circuit, tileBytes ' + tileBytes, ok && sameBits(got[0], golden.subarray(0, nt)) && sameBits(got[1], golden.subarray(nt)))
  }
  const withNaN = await lib.renderPiece(inTurn(spec.n), Object.assign(opts(0), { pans: Float32Array.from(spec.pans, (p) => (p === null ? NaN : p)) }))
  note('NaN in a Float32Array says what null says', withNaN.length === 2 && sameBits(withNaN[0], want.subarray(0, nt)) && sameBits(withNaN[1], want.subarray(nt)))
  const f32 = await lib.renderPiecePcm(inTurn(spec.n), Object.assign(opts(0), { bitDepth: 32 }))
  const frames = new Float32Array(f32.data.buffer, f32.data.byteOffset, f32.data.length / 4)
  let framesOk = f32.numberOfChannels === 2 && frames.length === 2 * nt
  for (let t = 0; framesOk && t < nt; t++) framesOk = Object.is(frames[2 * t], want[t]) && Object.is(frames[2 * t + 1], want[nt + t])
  note('renderPiecePcm f32 frames interleave the two channels', framesOk)
  const s16 = await lib.renderPiecePcm(inTurn(spec.n), Object.assign(opts(20000), { bitDepth: 16, normalise: 2 }))
  const wavFile = await lib.renderPieceWav(inTurn(spec.n), Object.assign(opts(20000), { bitDepth: 16, normalise: 2 }))
  note('renderPieceWav is the header and renderPiecePcm', wavFile.length === 44 + s16.data.length && s16.data.length === 4 * nt && wavFile.subarray(44).equals(s16.data) && Math.abs(s16.peak - spec.peak) === 0)
  // fractions: against Python's bits of the same call
  const fracWant = floatsOf(specPath.replace(/\.json$/, '.frac.f32'))
  const frac = await lib.renderPiece(inTurn(spec.n), Object.assign(opts(7000), { onsets: spec.fracOnsets, fracs: spec.fracs }))
  note('renderPiece stereo with fracs is Python\'s', frac.length === 2 && sameBits(frac[0], fracWant.subarray(0, nt)) && sameBits(frac[1], fracWant.subarray(nt)))
  // one kind of voice: the existing calls' bits
  const five = (kind) => Array.from({ length: 5 }, (_, k) => VOICES[kind](k))
  const few = { onsets: [0, 100, 200, 300, 400], duration: spec.duration }
  const wide = await lib.renderScore(five(2), Object.assign({ voiceDuration: spec.voiceDuration }, few))
  const wideStereo = await lib.renderScore(five(2), Object.assign({ voiceDuration: spec.voiceDuration, stereo: true }, few))
  note('two-channel voices: renderScore stereo is renderScore', wide.length === 2 && wideStereo.length === 2 && sameBits(wide[0], wideStereo[0]) && sameBits(wide[1], wideStereo[1]))
  const pans = [-1, 1, 0, 0.3, -0.7]
  const panned = await lib.renderPiece(five(0), Object.assign({ voiceDurations: spec.voiceDuration, pans }, few))
  const pannedStereo = await lib.renderPiece(five(0), Object.assign({ voiceDurations: spec.voiceDuration, pans, stereo: true }, few))
  note('panned mono voices: renderPiece stereo is renderPiece with pans', panned.length === 2 && sameBits(panned[0], pannedStereo[0]) && sameBits(panned[1], pannedStereo[1]))
  const mono = await lib.renderPiece(five(1), Object.assign({ voiceDurations: spec.voiceDuration }, few))
  const monoStereo = await lib.renderPiece(five(1), Object.assign({ voiceDurations: spec.voiceDuration, stereo: true }, few))
  note('plain mono voices: both channels are the mono piece', mono.length === 1 && monoStereo.length === 2 && sameBits(mono[0], monoStereo[0]) && sameBits(mono[0], monoStereo[1]))
  console.log(JSON.stringify(report))
}

const mode = process.argv.find((a) => a === 'refusals' || a === 'render')
const run = mode === 'refusals' ? refusals() : render(process.argv[process.argv.indexOf('render') + 1])
run.catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack ? e.stack : e) })); process.exit(1) })
