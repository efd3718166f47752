'use strict'
/* The `fracs` option of the JavaScript host (dusp_amd/js): voices of a score or piece placed between samples.
 *   node check_frac.js --sampleRate=48000 refusals
 *       no device: the refusal strings of renderPiece / renderScore and their Pcm / Wav forms with fracs, and splitOnsets, as one JSON
 *       line that tests/test_frac_host.py holds to Python's twin
 *   node check_frac.js --sampleRate=48000 render <spec.json>
 *       GPU: renderPiece / renderPiecePcm / renderScore with fracs of the list the spec describes against the bits Python's render_piece
 *       wrote to spec.f32 and against the oracle's one-circuit render (spec.golden), whatever tileBytes */
const fs = require('fs')
const lib = require('../../dusp_amd/js')
const rcd = require('../../dusp_amd/js/lib/renderChannelData')

const VOICES = { // twins of tests/score_voices.py voice, tests/test_piece_host.py saw_voice and tests/mix_voices.py voice
  score: (k) => new lib.Multiply(new lib.Osc(200.5 + 31 * k), new lib.Ramp(700, 1, 0).trigger()),
  saw: (k) => new lib.Multiply(new lib.Filter(new lib.Osc(110 + 3.25 * k, 'saw'), 900 + 40 * k), new lib.Ramp(1000, 1, 0).trigger()),
  filtered_saw: (k) => new lib.Filter(new lib.Osc(110 + 3.25 * k, 'saw'), 900 + 40 * k),
}
const interleaved = (n) => Array.from({ length: n }, (_, k) => VOICES[k % 2 === 0 ? 'score' : 'saw'](k >> 1))

async function rejection(f) {
  try { await f() } catch (e) { return typeof e === 'string' ? e : 'not a string: ' + e }
  return null
}

async function refusals() {
  const mono = () => [VOICES.score(0), VOICES.score(1), VOICES.score(2)]
  const two = () => [VOICES.score(0), VOICES.filtered_saw(0), VOICES.score(1)]
  const native = require('../../dusp_amd/js/lib/native')()
  const split = lib.splitOnsets([0, 5, -5, 5538.46153846, -0.25, -3.75, 1 / 3, 2 ** 51 + 0.5, -(2 ** 40) - 0.125])
  const report = {
    refusals: {
      shape: await rejection(() => lib.renderPiece(mono(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0.05, fracs: [0, 0] })),
      shapeScore: await rejection(() => lib.renderScore(mono(), { onsets: [0, 1, 2], voiceDuration: 0.01, duration: 0.05, fracs: [0, 0, 0, 0] })),
      finite: await rejection(() => lib.renderPiece(mono(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0.05, fracs: [0, 0.5, NaN] })),
      finitePcm: await rejection(() => lib.renderScorePcm(mono(), { onsets: [0, 1, 2], voiceDuration: 0.01, duration: 0.05, fracs: [0, 0.5, Infinity] })),
      finiteWav: await rejection(() => lib.renderScoreWav(mono(), { onsets: [0, 1, 2], voiceDuration: 0.01, duration: 0.05, pans: [0, 0, 0], fracs: [0, 0.5, -Infinity] })),
      range: await rejection(() => lib.renderPiece(mono(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0.05, fracs: [0, 1, 0.5] })),
      rangePcm: await rejection(() => lib.renderPiecePcm(mono(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0.05, fracs: [0, -0.5, 0.5] })),
      rangeWav: await rejection(() => lib.renderPieceWav(mono(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0, pans: [0, 0, 0], fracs: [0.999, 1.5, 7] })),
      onePart: await rejection(() => lib.renderScore(two(), { onsets: [0, 1, 2], voiceDuration: 0.01, duration: 0.05, fracs: [0, 0, 0] })),
    },
    whole: await rejection(() => lib.renderPiece(mono(), { onsets: [0, 0.5, 2], voiceDurations: 0.01, duration: 0.05, fracs: [0, 0.5, 0] })),
    addonCall: typeof native.renderPieceFrac === 'function',
    split: { onsets: Array.from(split.onsets), fracs: Array.from(split.fracs) },
    splitTiny: Array.from(lib.splitOnsets([-1e-300]).onsets).concat(Array.from(lib.splitOnsets([-1e-300]).fracs)),
    splitBad: await rejection(async () => lib.splitOnsets([0, NaN])),
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
  const want = floatsOf(specPath.replace(/\.json$/, '.f32')), golden = floatsOf(spec.golden) // planar [2][nTotal] each
  const nt = spec.nTotal
  const report = { failed: [], checked: 0 }
  const note = (name, ok) => { report.checked++; if (!ok) report.failed.push(name) }
  const opts = (tileBytes) => ({ onsets: spec.onsets, fracs: spec.fracs, gains: spec.gains, pans: spec.pans, voiceDurations: spec.voiceDurations, duration: spec.duration, tileBytes })
  note('the files hold two channels of the timeline', want.length === 2 * nt && golden.length === 2 * nt)
  for (const tileBytes of [0, 1, 20000]) {
    const got = await lib.renderPiece(interleaved(spec.n), opts(tileBytes))
    const ok = got.length === 2 && got.sampleRate === spec.sampleRate && got[0].length === nt
    note('renderPiece with fracs is Python\'s, tileBytes ' + tileBytes, ok && sameBits(got[0], want.subarray(0, nt)) && sameBits(got[1], want.subarray(nt)))
    note('renderPiece with fracs is the oracle\'s one circuit, tileBytes ' + tileBytes, ok && sameBits(got[0], golden.subarray(0, nt)) && sameBits(got[1], golden.subarray(nt)))
  }
  const positions = spec.onsets.map((on, k) => on + spec.fracs[k]) // (exact: onset + fraction is an f32 here)
  const split = lib.splitOnsets(positions)
  const viaSplit = await lib.renderPiece(interleaved(spec.n), Object.assign(opts(0), split))
  note('positions through splitOnsets give the same piece', viaSplit.length === 2 && sameBits(viaSplit[0], want.subarray(0, nt)) && sameBits(viaSplit[1], want.subarray(nt)))
  const rounded = await lib.renderPiece(interleaved(spec.n), Object.assign(opts(0), { fracs: undefined }))
  note('without fracs it is another piece', rounded.length === 2 && !sameBits(rounded[0], want.subarray(0, nt)))
  const zeros = await lib.renderPiece(interleaved(spec.n), Object.assign(opts(0), { fracs: new Float64Array(spec.n) }))
  note('all fractions zero is the piece without fracs', sameBits(zeros[0], rounded[0]) && sameBits(zeros[1], rounded[1]))
  const f32 = await lib.renderPiecePcm(interleaved(spec.n), Object.assign(opts(0), { bitDepth: 32 }))
  const frames = new Float32Array(f32.data.buffer, f32.data.byteOffset, f32.data.length / 4)
  let framesOk = f32.numberOfChannels === 2 && frames.length === 2 * nt
  for (let t = 0; framesOk && t < nt; t++) framesOk = Object.is(frames[2 * t], want[t]) && Object.is(frames[2 * t + 1], want[nt + t])
  note('renderPiecePcm f32 frames interleave the two channels', framesOk)
  const s16 = await lib.renderPiecePcm(interleaved(spec.n), Object.assign(opts(20000), { bitDepth: 16, normalise: 2 }))
  const wavFile = await lib.renderPieceWav(interleaved(spec.n), Object.assign(opts(20000), { bitDepth: 16, normalise: 2 }))
  note('renderPieceWav is the header and renderPiecePcm', wavFile.length === 44 + s16.data.length && s16.data.length === 4 * nt && wavFile.subarray(44).equals(s16.data) && Math.abs(s16.peak - spec.peak) === 0)
  const five = () => Array.from({ length: 5 }, (_, k) => VOICES.score(k))
  const few = { onsets: [0, 100, 200, 300, 400], fracs: [0, 0.25, 0.5, 0.75, 0.125], duration: spec.duration }
  const one = await lib.renderPiece(five(), Object.assign({ voiceDurations: spec.voiceDurations[0] }, few))
  const score = await lib.renderScore(five(), Object.assign({ voiceDuration: spec.voiceDurations[0] }, few))
  note('renderScore with fracs is renderPiece of one structure, mono', one.length === 1 && score.length === 1 && sameBits(one[0], score[0]))
  const plain = await lib.renderScore(five(), { onsets: few.onsets, voiceDuration: spec.voiceDurations[0], duration: spec.duration })
  note('and not the score without fracs', plain.length === 1 && !sameBits(plain[0], score[0]))
  console.log(JSON.stringify(report))
}

const mode = process.argv.find((a) => a === 'refusals' || a === 'render')
const run = mode === 'refusals' ? refusals() : render(process.argv[process.argv.indexOf('render') + 1])
run.catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack ? e.stack : e) })); process.exit(1) })
