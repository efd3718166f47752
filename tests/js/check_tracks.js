'use strict'
/* Tracks in the JavaScript host (dusp_amd/js): the `tracks`, `trackOf`, `faders` and `trackSends` options of renderPiece / renderScore.
 *   node check_tracks.js --sampleRate=48000 surface
 *       no device: the refusal strings of tracks and of a track's circuit, checkTracks' arrays and trackPrograms' groups, as one JSON
 *       line that tests/test_js_tracks.py holds to Python's twin (mix.check_tracks, render.track_programs, mix.TRACK_*, mix.TRACKS_*)
 *   node check_tracks.js --sampleRate=48000 render <spec.json>
 *       GPU: renderPiece / renderPiecePcm / renderScore with tracks against the bits Python's render_piece wrote */
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
  const refuse = (track, channels) => rejection(() => rcd.trackPrograms([null, track], channels, rate))
  const mono = () => [VOICES.score(0), VOICES.score(1), VOICES.score(2)]
  const of = [0, -1, 0], two = [clip, null]
  const piece = (extra) => rejection(() => lib.renderPiece(mono(), Object.assign({ onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0 }, extra)))
  const checked = rcd.checkTracks(3, 2, [0, -1, 1], [0.5, 2], [[0, 1], [1, 0.25]], 2)
  const groups = rcd.trackPrograms([echoOf(300.25), clip, null, echoOf(411.5), [echoOf(100.5)], clip], 1, rate)
  const wide = rcd.trackPrograms([[echoOf(300.25), echoOf(411.5)], echoOf(100.5)], 2, rate)
  const report = {
    trackOf: Array.from(checked.trackOf), faders: Array.from(checked.faders), trackSends: Array.from(checked.trackSends),
    oneBus: Array.from(rcd.checkTracks(3, 2, Int32Array.of(0, -1, 1), null, [0.5, 1], 1).trackSends),
    none: rcd.checkTracks(3, null, null),
    groups: groups.map((g) => ({ tracks: g.tracks, nInstances: g.uni.nInstances, params: g.uni.nParams ? Array.from(g.uni.params) : [] })),
    wide: wide.map((g) => ({ tracks: g.tracks, nInstances: g.uni.nInstances, params: Array.from(g.uni.params) })),
    track: {
      notCallable: await refuse(5, 1),
      emptyList: await refuse([], 1),
      count: await refuse([echo], 2),
      noInput: await refuse(() => VOICES.score(0), 1),
      hostSource: await refuse((x) => new lib.Sum(x, new lib.Noise()), 1),
      events: await refuse(scheduled, 1),
      channels: await refuse((x) => new lib.Pan(x, 0.25), 1),
      notIsomorphic: await refuse([echo, clip], 2),
    },
    tracks: {
      trackOfAlone: await piece({ trackOf: of }),
      fadersAlone: await piece({ faders: [1] }),
      sendsAlone: await piece({ trackSends: [[1]] }),
      withoutTrackOf: await piece({ tracks: [clip] }),
      none: await piece({ tracks: [], trackOf: of }),
      nine: await piece({ tracks: new Array(9).fill(null), trackOf: of }),
      notAList: await piece({ tracks: clip, trackOf: of }),
      short: await piece({ tracks: two, trackOf: [0, 1] }),
      notWhole: await piece({ tracks: two, trackOf: [0, 0.5, 1] }),
      tooHigh: await piece({ tracks: two, trackOf: [0, 2, 1] }),
      tooLow: await piece({ tracks: two, trackOf: [0, 1, -2] }),
      fadersShape: await piece({ tracks: two, trackOf: of, faders: [1] }),
      faderNaN: await piece({ tracks: two, trackOf: of, faders: [1, NaN] }),
      faderTooLarge: await piece({ tracks: two, trackOf: of, faders: [1e39, 1] }),
      sendsWithoutBuses: await piece({ tracks: two, trackOf: of, trackSends: [[1, 1]] }),
      busesWithoutSends: await piece({ tracks: two, trackOf: of, buses: [echo] }),
      withSends: await piece({ tracks: two, trackOf: of, buses: [echo], sends: [1, 1, 1] }),
      withBoth: await piece({ tracks: two, trackOf: of, buses: [echo], sends: [1, 1, 1], trackSends: [[1, 1]] }),
      noBuses: await piece({ tracks: two, trackOf: of, buses: [], trackSends: [[1, 1]] }),
      fiveBuses: await piece({ tracks: two, trackOf: of, buses: [echo, echo, echo, echo, echo], trackSends: [[1, 1], [1, 1], [1, 1], [1, 1], [1, 1]] }),
      sendsShape: await piece({ tracks: two, trackOf: of, buses: [echo], trackSends: [[1, 1, 1]] }),
      oneRowForTwo: await piece({ tracks: two, trackOf: of, buses: [echo, comb], trackSends: [1, 1] }),
      levelNotFinite: await piece({ tracks: two, trackOf: of, buses: [echo, comb], trackSends: [[1, 1], [Infinity, 1]] }),
      // ... and through every call that takes the options
      score: await rejection(() => lib.renderScore(mono(), { onsets: [0, 1, 2], voiceDuration: 0.01, duration: 0, trackOf: of })),
      piecePcm: await rejection(() => lib.renderPiecePcm(mono(), { onsets: [0, 1, 2], voiceDurations: 0.01, duration: 0, trackOf: of })),
      scoreWav: await rejection(() => lib.renderScoreWav(mono(), { onsets: [0, 1, 2], voiceDuration: 0.01, duration: 0, trackOf: of })),
      badTrackInACall: await piece({ tracks: [echo, 5], trackOf: [0, 1, -1] }),
    },
    // with tracks the buses are fed by the tracks: every placement goes with them
    noSamples: [(await lib.renderPiece(mono(), { onsets: [1, 2, 3], voiceDurations: 0.01, duration: 0, tracks: two, trackOf: of, buses: [echo], trackSends: [1, 0], fracs: [0, 0.5, 0] })).length,
      (await lib.renderPiece(mono(), { onsets: [1, 2, 3], voiceDurations: 0.01, duration: 0, tracks: two, trackOf: of, buses: [echo], trackSends: [1, 0], stereo: true })).length,
      (await lib.renderScore(mono(), { onsets: [1, 2, 3], voiceDuration: 0.01, duration: 0, tracks: two, trackOf: of, faders: [1, 0.5] })).length],
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
  const want = file(''), wantThree = file('.three'), wantPan = file('.pan'), wantScore = file('.score'), wantFull = file('.full')
  const report = { failed: [], checked: 0 }
  const note = (name, ok) => { report.checked++; if (!ok) report.failed.push(name) }
  const opts = (tileBytes, extra) => Object.assign({ onsets: spec.onsets, gains: spec.gains, voiceDurations: spec.voiceDurations, duration: spec.duration, tileBytes,
    tracks: [clip, echo], trackOf: spec.trackOf2, faders: spec.faders2 }, extra)
  for (const tileBytes of [0, 9000]) {
    const got = await lib.renderPiece(interleaved(spec.n), opts(tileBytes))
    note('renderPiece with a clip and an echo track, tileBytes ' + tileBytes, got.length === 1 && got.sampleRate === spec.sampleRate && sameBits(got[0], want))
  }
  const plain = await lib.renderPiece(interleaved(spec.n), opts(0, { tracks: undefined, trackOf: undefined, faders: undefined }))
  note('the tracks change the piece', !sameBits(plain[0], want))
  // three echoes at three delays (one program), no faders
  const three = await lib.renderPiece(interleaved(spec.n), opts(0, { tracks: [echoOf(300.25), echoOf(411.5), echoOf(257.75)], trackOf: spec.trackOf3, faders: undefined }))
  note('three echo tracks as one program', three.length === 1 && sameBits(three[0], wantThree))
  // a clip, a fader group and an echo; buses fed by the tracks, one level column all zero; a master behind them
  const full = await lib.renderPiece(interleaved(spec.n), opts(9000, { tracks: [clip, null, echo], trackOf: spec.trackOf3, faders: spec.faders3, buses: [echo, comb],
    trackSends: spec.trackSends, master: comb }))
  note('tracks, buses and a master', full.length === 1 && sameBits(full[0], wantFull))
  const f32 = await lib.renderPiecePcm(interleaved(spec.n), opts(0, { bitDepth: 32 }))
  note('renderPiecePcm f32 frames', f32.numberOfChannels === 1 && sameBits(new Float32Array(f32.data.buffer, f32.data.byteOffset, f32.data.length / 4), want))
  const s16 = await lib.renderPiecePcm(interleaved(spec.n), opts(9000, { bitDepth: 16, normalise: 2 }))
  const wavFile = await lib.renderPieceWav(interleaved(spec.n), opts(9000, { bitDepth: 16, normalise: 2 }))
  note('renderPieceWav is the header and renderPiecePcm', wavFile.length === 44 + s16.data.length && wavFile.subarray(44).equals(s16.data) && Math.abs(s16.peak - spec.peak) === 0)
  // panned mono voices with fractions, a track circuit a channel, a bus behind them
  const score5 = () => Array.from({ length: 5 }, (_, k) => VOICES.score(k))
  const five = { onsets: spec.fiveOnsets, gains: spec.fiveGains, duration: spec.duration }
  const pan = await lib.renderPiece(score5(), Object.assign({ voiceDurations: spec.voiceDurations[0], pans: spec.pans, fracs: spec.fiveFracs,
    tracks: [[echoOf(300.25), echoOf(411.5)], null], trackOf: spec.fiveTrackOf, faders: spec.faders2, buses: [clip], trackSends: [spec.fiveLevels] }, five))
  note('pans and fracs, a track circuit a channel, a bus', pan.length === 2 && sameBits(pan[0], wantPan.subarray(0, want.length)) && sameBits(pan[1], wantPan.subarray(want.length)))
  // a score with tracks goes the piece's way
  const score = await lib.renderScore(score5(), Object.assign({ voiceDuration: spec.voiceDurations[0], tracks: [echo, comb], trackOf: spec.fiveTrackOf, faders: spec.faders2 }, five))
  note('renderScore with tracks', score.length === 1 && sameBits(score[0], wantScore))
  console.log(JSON.stringify(report))
}

const mode = process.argv.find((a) => a === 'surface' || a === 'render')
const run = mode === 'surface' ? surface() : render(process.argv[process.argv.indexOf('render') + 1])
run.catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack ? e.stack : e) })); process.exit(1) })
