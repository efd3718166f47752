'use strict'
/* renderPiece of the JavaScript host (dusp_amd/js): a voice list of several structures and lengths as ONE chain on the device.
 *   node check_piece.js --sampleRate=48000 grouping
 *       no device: the grouping of a mixed voice list into parts (pieceParts), the channel counts of its descriptors and the
 *       refusal strings, as one JSON line that tests/test_js_piece.py holds to Python's twin
 *   node check_piece.js --sampleRate=48000 render <spec.json>
 *       GPU: renderPiece / renderPiecePcm of the list the spec describes against the bits Python's render_piece wrote to spec.f32,
 *       whatever tileBytes */
const fs = require('fs')
const lib = require('../../dusp_amd/js')
const { extract } = require('../../dusp_amd/js/lib/extract')
const rcd = require('../../dusp_amd/js/lib/renderChannelData')

const VOICES = { // twins of tests/score_voices.py voice, tests/test_piece_host.py saw_voice and tests/mix_voices.py voice
  score: (k) => new lib.Multiply(new lib.Osc(200.5 + 31 * k), new lib.Ramp(700, 1, 0).trigger()),
  saw: (k) => new lib.Multiply(new lib.Filter(new lib.Osc(110 + 3.25 * k, 'saw'), 900 + 40 * k), new lib.Ramp(1000, 1, 0).trigger()),
  filtered_saw: (k) => new lib.Filter(new lib.Osc(110 + 3.25 * k, 'saw'), 900 + 40 * k),
  pan: (k) => new lib.Pan(new lib.Osc(200 + 7 * k, 'triangle'), -0.9 + 0.025 * k),
}
const interleaved = (n) => Array.from({ length: n }, (_, k) => VOICES[k % 2 === 0 ? 'score' : 'saw'](k >> 1))

async function rejection(f) {
  try { await f() } catch (e) { return typeof e === 'string' ? e : 'not a string: ' + e }
  return null
}

async function grouping() {
  const kinds = ['score', 'filtered_saw', 'score', 'pan', 'filtered_saw', 'score', 'filtered_saw', 'score']
  const samples = [773, 1031, 773, 500, 1031, 400, 1031, 773]
  const made = {}
  const extractions = kinds.map((kind) => { made[kind] = (made[kind] || 0) + 1; return extract(VOICES[kind](made[kind] - 1)) })
  const g = rcd.pieceParts(extractions, samples)
  const keys = extractions.map(rcd.structureKey)
  const native = require('../../dusp_amd/js/lib/native')()
  const mixed = () => [VOICES.score(0), VOICES.pan(0), VOICES.score(1)]
  const report = {
    partOf: Array.from(g.partOf), instanceOf: g.instanceOf, sampleRate: g.sampleRate,
    parts: g.parts.map((p) => [p.uni.nInstances, p.nVoiceSamples, p.uni.nParams]),
    words: g.parts.map((p) => Array.from(p.uni.words, (w) => (Number.isNaN(w) ? 'nan' : w))),
    params: g.parts.map((p) => (p.uni.nParams ? Array.from(p.uni.params) : null)),
    keysAlike: keys[0] === keys[2] && keys[0] === keys[5] && keys[1] === keys[4], keysApart: new Set([keys[0], keys[1], keys[3]]).size === 3,
    channels: [native.descriptorChannels(extractions[0].words), native.descriptorChannels(extractions[3].words)],
    refusals: {
      channels: await rejection(() => lib.renderPiece(mixed(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0.05 })),
      channelsPcm: await rejection(() => lib.renderPiecePcm(mixed(), { onsets: [0, 1, 2], voiceDurations: [0.01, 0.02, 0.01], duration: 0.05 })),
      channelsWav: await rejection(() => lib.renderPieceWav(mixed(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0 })),
      check: await rejection(() => rcd.checkPieceChannels([1, 2, 1])),
      none: await rejection(() => rcd.pieceParts([], [])),
      fraction: await rejection(() => lib.renderPiece([VOICES.score(0), VOICES.score(1)], { onsets: [0, 0.5], voiceDurations: 0.01, duration: 0.05 })),
      durations: await rejection(() => lib.renderPiece([VOICES.score(0), VOICES.score(1)], { onsets: [0, 1], voiceDurations: [0.01], duration: 0.05 })),
      lengths: await rejection(() => lib.renderPiece([VOICES.score(0), VOICES.score(1)], { onsets: [0, 1], voiceDurations: [0.01, 0.02], duration: 0.05, lengths: [480, 961] })),
      noSample: await rejection(() => lib.renderPiece([VOICES.score(0), VOICES.score(1)], { onsets: [0, 1], voiceDurations: [0.01, 0], duration: 0.05 })),
    },
  }
  console.log(JSON.stringify(report))
}

function sameBits(a, b) {
  if (a.length !== b.length) return false
  const x = new Uint32Array(a.buffer, a.byteOffset, a.length), y = new Uint32Array(b.buffer, b.byteOffset, b.length)
  for (let t = 0; t < x.length; t++) if (x[t] !== y[t]) return false
  return true
}

async function render(specPath) {
  const spec = JSON.parse(fs.readFileSync(specPath, 'utf8'))
  const raw = fs.readFileSync(specPath.replace(/\.json$/, '.f32'))
  const want = new Float32Array(raw.buffer, raw.byteOffset, raw.length / 4)
  const report = { failed: [], checked: 0 }
  const note = (name, ok) => { report.checked++; if (!ok) report.failed.push(name) }
  const opts = (tileBytes) => ({ onsets: spec.onsets, lengths: spec.lengths, gains: spec.gains, voiceDurations: spec.voiceDurations, duration: spec.duration, tileBytes })
  for (const tileBytes of [0, 1, 20000]) {
    const got = await lib.renderPiece(interleaved(spec.n), opts(tileBytes))
    note('renderPiece tileBytes ' + tileBytes, got.length === 1 && got.sampleRate === spec.sampleRate && sameBits(got[0], want))
  }
  const f32 = await lib.renderPiecePcm(interleaved(spec.n), Object.assign(opts(0), { bitDepth: 32 }))
  note('renderPiecePcm f32 frames', f32.numberOfChannels === 1 && sameBits(new Float32Array(f32.data.buffer, f32.data.byteOffset, f32.data.length / 4), want))
  const s16 = await lib.renderPiecePcm(interleaved(spec.n), Object.assign(opts(20000), { bitDepth: 16, normalise: 2 }))
  const wavFile = await lib.renderPieceWav(interleaved(spec.n), Object.assign(opts(20000), { bitDepth: 16, normalise: 2 }))
  note('renderPieceWav is the header and renderPiecePcm', wavFile.length === 44 + s16.data.length && wavFile.subarray(44).equals(s16.data) && Math.abs(s16.peak - spec.peak) === 0)
  const one = await lib.renderPiece(Array.from({ length: 5 }, (_, k) => VOICES.score(k)), { onsets: [0, 100, 200, 300, 400], voiceDurations: spec.voiceDurations[0], duration: spec.duration })
  const score = await lib.renderScore(Array.from({ length: 5 }, (_, k) => VOICES.score(k)), { onsets: [0, 100, 200, 300, 400], voiceDuration: spec.voiceDurations[0], duration: spec.duration })
  note('one structure and one duration is renderScore', sameBits(one[0], score[0]))
  console.log(JSON.stringify(report))
}

const mode = process.argv.find((a) => a === 'grouping' || a === 'render')
const run = mode === 'grouping' ? grouping() : render(process.argv[process.argv.indexOf('render') + 1])
run.catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack ? e.stack : e) })); process.exit(1) })
