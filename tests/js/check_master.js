'use strict'
/* The master of a score or piece in the JavaScript host (dusp_amd/js): the `master` option of renderPiece / renderScore.
 *   node check_master.js --sampleRate=48000 surface
 *       no device: the refusal strings of a master and the unified master's parameter table, as one JSON line that
 *       tests/test_js_master.py holds to Python's twin (render.master_program, mix.MASTER_*)
 *   node check_master.js --sampleRate=48000 render <spec.json>
 *       GPU: renderPiece / renderPiecePcm / renderScore with a master against the bits Python's render_piece wrote (spec.f32: the mono
 *       piece behind the echo; spec.stereo.f32: two channels, an echo of its own per channel) */
const fs = require('fs')
const lib = require('../../dusp_amd/js')
const rcd = require('../../dusp_amd/js/lib/renderChannelData')

const VOICES = { // twins of tests/score_voices.py voice, tests/test_piece_host.py saw_voice and tests/stereo_cases.py voice(k, TWO)
  score: (k) => new lib.Multiply(new lib.Osc(200.5 + 31 * k), new lib.Ramp(700, 1, 0).trigger()),
  saw: (k) => new lib.Multiply(new lib.Filter(new lib.Osc(110 + 3.25 * k, 'saw'), 900 + 40 * k), new lib.Ramp(1000, 1, 0).trigger()),
  stereo: (k) => new lib.Multiply(VOICES.score(k), [0.75 - 0.03125 * (k % 5), -0.5 + 0.0625 * (k % 7)]),
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
const scheduled = (x) => { const u = clip(x); u.schedule(0.01, () => {}); return u }

async function rejection(f) {
  try { await f() } catch (e) { return typeof e === 'string' ? e : 'not a string: ' + e }
  return null
}

async function surface() {
  const rate = lib.config.sampleRate
  const refuse = (master, channels) => rejection(() => rcd.masterProgram(master, channels, rate))
  const two = rcd.masterProgram([echoOf(300.25), echoOf(411.5)], 2, rate), one = rcd.masterProgram(echo, 3, rate)
  const mono = () => [VOICES.score(0), VOICES.score(1), VOICES.score(2)]
  const report = {
    two: { nParams: two.nParams, nInstances: two.nInstances, params: Array.from(two.params), words: Array.from(two.words, (w) => (Number.isNaN(w) ? 'nan' : w)) },
    one: { nParams: one.nParams, nInstances: one.nInstances },
    refusals: {
      notCallable: await refuse(5, 1),
      emptyList: await refuse([], 1),
      count: await refuse([echo], 2),
      noInput: await refuse(() => VOICES.score(0), 1),
      twoInputs: await refuse([echo, (x) => new lib.Sum(x, new lib.MasterInput())], 2),
      hostSource: await refuse((x) => new lib.Sum(x, new lib.Noise()), 1),
      events: await refuse(scheduled, 1),
      channels: await refuse((x) => new lib.Pan(x, 0.25), 1),
      notIsomorphic: await refuse([echo, echo, clip], 3),
      inputAlone: await rejection(() => lib.renderChannelData(clip(new lib.MasterInput()), 0.01)),
      // ... and through every call that takes the option, before anything is built (a timeline of no samples needs no device)
      piece: await rejection(() => lib.renderPiece(mono(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0, master: 5 })),
      score: await rejection(() => lib.renderScore(mono(), { onsets: [0, 1, 2], voiceDuration: 0.01, duration: 0, master: 5 })),
      piecePcm: await rejection(() => lib.renderPiecePcm(mono(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0, master: 5 })),
      scoreWav: await rejection(() => lib.renderScoreWav(mono(), { onsets: [0, 1, 2], voiceDuration: 0.01, duration: 0, master: 5 })),
    },
    noSamples: (await lib.renderPiece(mono(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0, master: echo })).length,
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
  const want = f32File(specPath.replace(/\.json$/, '.f32')), wantStereo = f32File(specPath.replace(/\.json$/, '.stereo.f32'))
  const wantScore = f32File(specPath.replace(/\.json$/, '.score.f32'))
  const report = { failed: [], checked: 0 }
  const note = (name, ok) => { report.checked++; if (!ok) report.failed.push(name) }
  const opts = (tileBytes) => ({ onsets: spec.onsets, gains: spec.gains, voiceDurations: spec.voiceDurations, duration: spec.duration, tileBytes, master: echo })
  for (const tileBytes of [0, 9000]) {
    const got = await lib.renderPiece(interleaved(spec.n), opts(tileBytes))
    note('renderPiece with a master, tileBytes ' + tileBytes, got.length === 1 && got.sampleRate === spec.sampleRate && sameBits(got[0], want))
  }
  const plain = await lib.renderPiece(interleaved(spec.n), Object.assign(opts(0), { master: undefined }))
  note('the master changes the piece', !sameBits(plain[0], want))
  const f32 = await lib.renderPiecePcm(interleaved(spec.n), Object.assign(opts(0), { bitDepth: 32 }))
  note('renderPiecePcm f32 frames', f32.numberOfChannels === 1 && sameBits(new Float32Array(f32.data.buffer, f32.data.byteOffset, f32.data.length / 4), want))
  const s16 = await lib.renderPiecePcm(interleaved(spec.n), Object.assign(opts(9000), { bitDepth: 16, normalise: 2 }))
  const wavFile = await lib.renderPieceWav(interleaved(spec.n), Object.assign(opts(9000), { bitDepth: 16, normalise: 2 }))
  note('renderPieceWav is the header and renderPiecePcm', wavFile.length === 44 + s16.data.length && wavFile.subarray(44).equals(s16.data) && Math.abs(s16.peak - spec.peak) === 0)
  // two channels, an echo of its own per channel: one program, the delay its parameter
  const stereo = await lib.renderPiece(Array.from({ length: 5 }, (_, k) => VOICES.stereo(k)),
    { onsets: spec.stereoOnsets, gains: spec.stereoGains, voiceDurations: spec.voiceDurations[0], duration: spec.duration, master: [echoOf(300.25), echoOf(411.5)] })
  note('two channels, a master a channel', stereo.length === 2 && sameBits(stereo[0], wantStereo.subarray(0, want.length)) && sameBits(stereo[1], wantStereo.subarray(want.length)))
  // a score with a master goes the piece's way
  const score = await lib.renderScore(Array.from({ length: 5 }, (_, k) => VOICES.score(k)),
    { onsets: spec.stereoOnsets, gains: spec.stereoGains, voiceDuration: spec.voiceDurations[0], duration: spec.duration, master: echo })
  note('renderScore with a master', score.length === 1 && sameBits(score[0], wantScore))
  console.log(JSON.stringify(report))
}

const mode = process.argv.find((a) => a === 'surface' || a === 'render')
const run = mode === 'surface' ? surface() : render(process.argv[process.argv.indexOf('render') + 1])
run.catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack ? e.stack : e) })); process.exit(1) })
