'use strict'
/* renderScore / renderScorePcm / renderScoreWav (GPU): voices mixed on the device at per-voice onsets, against the Math.fround chain over
 * renderMany's rows placed at their onsets — bit for bit — and, for the score voice (which the device renders bit for bit), against
 * renderChannelData(Sum.many(voices.map((v, k) => new Delay(v, onset_k, 4096)))); gains, lengths, negative onsets, a stereo voice,
 * tiles, the ways onsets may be given, the encoded forms and the rejection strings.
 *   node check_score.js --sampleRate=48000 */
const lib = require('../../dusp_amd/js')
const SR = lib.config.sampleRate
const NT = 2317, NV = 773
const DUR = (NT + 0.5) / SR, VOICE_DUR = (NV + 0.5) / SR // (durations are in seconds and truncate to these sample counts)

const VOICES = {
  score: (k) => new lib.Multiply(new lib.Osc(200.5 + 31 * k), new lib.Ramp(700, 1, 0).trigger()), // ends in zeros by sample 700
  pan: (k) => new lib.Pan(new lib.Osc(200 + 7 * k), -0.9 + 0.05 * k), // two channels; held to renderMany's own voices
  filtered: (k) => new lib.Filter(new lib.Osc(110 + 3.25 * k), 900 + 40 * k),
}
const voices = (kind, n) => Array.from({ length: n }, (_, k) => VOICES[kind](k))
function layout(n) {
  let x = 12345 + n
  const next = (lo, hi) => { x = (x * 1103515245 + 12345) % 2147483648; return lo + (x >> 8) % (hi - lo) }
  const onsets = Array.from({ length: n }, () => next(1, NT - 10)), lengths = Array.from({ length: n }, () => next(700, NV + 1))
  onsets[n >> 1] = 0
  const gains = Float32Array.from({ length: n }, (_, k) => Math.fround(0.1 + 1.7 * ((k * 37) % 11) / 11))
  if (n > 2) gains[1] = -gains[1]
  return { onsets, lengths, gains }
}

/* the contract, in JavaScript: many[instance][channel] -> [channel] Float32Array of nTotal samples */
function chain(many, onsets, nTotal, lengths, gains) {
  return many[0].map((_, c) => {
    const out = new Float32Array(nTotal)
    for (let t = 0; t < nTotal; t++) {
      let acc = 0
      for (let i = 0; i < many.length; i++) {
        const s = t - onsets[i]
        if (s < 0 || s >= (lengths ? lengths[i] : many[i][c].length)) continue
        acc = Math.fround(acc + (gains ? Math.fround(many[i][c][s] * gains[i]) : many[i][c][s]))
      }
      out[t] = acc || 0
    }
    return out
  })
}
function sameBits(a, b) {
  if (a.length !== b.length) return false
  for (let c = 0; c < a.length; c++) {
    if (a[c].length !== b[c].length) return false
    const x = new Uint32Array(a[c].buffer, a[c].byteOffset, a[c].length), y = new Uint32Array(b[c].buffer, b[c].byteOffset, b[c].length)
    for (let t = 0; t < x.length; t++) if (x[t] !== y[t]) return false
  }
  return true
}

async function main() {
  const report = { failed: [], checked: 0 }
  const note = (name, ok, extra) => { report.checked++; if (!ok) report.failed.push(Object.assign({ name }, extra)) }

  for (const kind of Object.keys(VOICES))
    for (const n of [1, 2, 13, 37]) {
      const { onsets, lengths, gains } = layout(n)
      const many = await lib.renderMany(voices(kind, n), VOICE_DUR, { devices: [0] })
      note(kind + ' x' + n + ' voice length', many[0][0].length === NV)
      const piece = await lib.renderScore(voices(kind, n), { onsets, lengths, voiceDuration: VOICE_DUR, duration: DUR })
      note(kind + ' x' + n + ' == chain over renderMany', piece.sampleRate === SR && piece.length === (kind === 'pan' ? 2 : 1) && piece[0].length === NT &&
        sameBits(piece, chain(many, onsets, NT, lengths)))
      const pieceG = await lib.renderScore(voices(kind, n), { onsets: BigInt64Array.from(onsets.map(BigInt)), voiceDuration: VOICE_DUR, duration: DUR, gains, tileInstances: 5 })
      note(kind + ' x' + n + ' gains, no lengths, tiles of 5, BigInt64Array', sameBits(pieceG, chain(many, onsets, NT, null, gains)))
      if (kind === 'score') {
        const delayed = (vs) => lib.Sum.many(vs.map((v, k) => onsets[k] === 0 ? v : new lib.Delay(v, onsets[k], 4096)))
        note('score x' + n + ' == Sum.many of Delays', sameBits(piece, await lib.renderChannelData(delayed(voices(kind, n)), DUR)))
        const oneG = await lib.renderChannelData(delayed(voices(kind, n).map((v, k) => new lib.Multiply(v, gains[k]))), DUR)
        note('score x' + n + ' gains == Sum.many of Delays of Multiply', sameBits(pieceG, oneG))
      }
    }
  { // tiles, engines, negative onsets and onsets past the end, and the ways to give them: the same bits
    const n = 37, { onsets, lengths } = layout(n)
    const shifted = onsets.map((o, k) => k % 5 === 0 ? o - 400 : k % 7 === 0 ? o + NT : o)
    const many = await lib.renderMany(voices('score', n), VOICE_DUR, { devices: [0] })
    const want = chain(many, shifted, NT, lengths)
    const opts = { onsets: shifted, lengths, voiceDuration: VOICE_DUR, duration: DUR }
    const ref = await lib.renderScore(voices('score', n), opts)
    note('negative onsets and onsets past the end', sameBits(ref, want))
    for (const tileInstances of [1, 3, 64]) note('tile ' + tileInstances, sameBits(await lib.renderScore(voices('score', n), Object.assign({ tileInstances }, opts)), ref))
    note('chunk engine', sameBits(await lib.renderScore(voices('score', n), Object.assign({ engine: 1 }, opts)), ref))
    note('Float64Array onsets', sameBits(await lib.renderScore(voices('score', n), Object.assign({}, opts, { onsets: Float64Array.from(shifted), lengths: Float64Array.from(lengths) })), ref))
    note('BigInt onsets in a plain array', sameBits(await lib.renderScore(voices('score', n), Object.assign({}, opts, { onsets: shifted.map(BigInt) })), ref))
    note('no samples', (await lib.renderScore(voices('score', 3), { onsets: [0, 1, 2], duration: 0 })).length === 0)
  }
  // the encoded forms: the host encoder over the f32 piece, and a file that decodes to the same frames
  for (const kind of ['pan', 'score'])
    for (const bitDepth of [16, 24, 32]) {
      const n = 37, { onsets, lengths } = layout(n)
      const opts = { onsets, lengths, voiceDuration: VOICE_DUR, duration: DUR }
      const piece = await lib.renderScore(voices(kind, n), opts)
      const planar = new Float32Array(piece.length * NT)
      piece.forEach((ch, c) => planar.set(ch, c * NT))
      const host = lib.encodeFrames(planar, piece.length, NT, bitDepth, 2)
      const pcm = await lib.renderScorePcm(voices(kind, n), Object.assign({ bitDepth, normalise: 2 }, opts))
      note('renderScorePcm ' + kind + ' ' + bitDepth, pcm.data.equals(host.data) && pcm.peak === host.peak && pcm.peak > 0 && pcm.numberOfChannels === piece.length && pcm.bitDepth === bitDepth && pcm.sampleRate === SR,
        { peak: pcm.peak, want: host.peak })
      const file = await lib.renderScoreWav(voices(kind, n), Object.assign({ bitDepth }, opts))
      note('renderScoreWav ' + kind + ' ' + bitDepth, file.equals(lib.encodeWav(piece, { bitDepth })))
      const back = lib.decodeWav(file)
      note('renderScoreWav decodes ' + kind + ' ' + bitDepth, back.numberOfChannels === piece.length && back.bitDepth === bitDepth && back.sampleRate === SR && back.channelData[0].length === NT &&
        (bitDepth !== 32 || sameBits(back.channelData, piece)))
    }
  // what is refused, with strings
  const rejections = []
  const refused = (p) => p.then(() => rejections.push(null), (e) => rejections.push(e))
  const three = () => voices('score', 3)
  await refused(lib.renderScore([new lib.Multiply(new lib.Noise(), 0.5), new lib.Multiply(new lib.Noise(), 0.25)], { onsets: [0, 1], duration: DUR })) // ticks on the host
  note('a Noise voice', typeof rejections[0] === 'string' && rejections[0].startsWith('dusp-hip: renderScore does not take circuits with host-ticked units'), { got: rejections[0] })
  const evented = (k) => { const v = new lib.Multiply(new lib.Osc(330 + k), 1.5); v.schedule(0.01, function () { this.B = 0.75 }); return v }
  await refused(lib.renderScore([evented(0), evented(1)], { onsets: [0, 1], duration: DUR }))
  await refused(lib.renderScore(three(), { duration: DUR }))                                          // no onsets
  await refused(lib.renderScore(three(), { onsets: [0, 1], duration: DUR }))                          // one short
  await refused(lib.renderScore(three(), { onsets: [0, 1.5, 2], duration: DUR }))                     // a fraction
  await refused(lib.renderScore(three(), { onsets: Float64Array.of(0, NaN, 2), duration: DUR }))
  await refused(lib.renderScore(three(), { onsets: new Int32Array(3), duration: DUR }))               // another kind of array
  await refused(lib.renderScore(three(), { onsets: [0, 1, 2], lengths: [1, 2.5, 3], duration: DUR }))
  await refused(lib.renderScore(three(), { onsets: [0, 1, 2], lengths: [1, 2], duration: DUR }))
  await refused(lib.renderScore(three(), { onsets: [0, 1, 2], lengths: [1, 2, NV + 1], voiceDuration: VOICE_DUR, duration: DUR })) // (the library's refusal)
  await refused(lib.renderScore(three(), { onsets: [0, 1, 2], lengths: [1, -2, 3], voiceDuration: VOICE_DUR, duration: DUR }))
  await refused(lib.renderScore(three(), { onsets: [0, 1, 2], voiceDuration: 0, duration: DUR }))
  await refused(lib.renderScore(three(), { onsets: [0, 1, 2], duration: DUR, gains: [1, 2] }))
  await refused(lib.renderScore(three(), { onsets: [0, 1, 2], duration: DUR, tileInstances: 1.5 }))
  await refused(lib.renderScorePcm(three(), { onsets: [0, 1, 2], duration: DUR, bitDepth: 8 }))
  await refused(lib.renderScoreWav(three(), { onsets: [0, 1, 2], duration: DUR, normalise: 3 }))
  note('rejections', rejections.length === 16 && rejections.every((e) => typeof e === 'string' && e.startsWith('dusp-hip:')), { rejections })
  note('a length past the voice names the voice', /voice 2/.test(rejections[9]) && /lengths/.test(rejections[9]), { got: rejections[9] })
  // ... and the addon itself
  const native = require('../../dusp_amd/js/lib/native')()
  const uni = lib.unify(voices('score', 4).map((v) => lib.extract(v)))
  const ctx = native.ctxCreate(-1)
  require('../../dusp_amd/js/lib/wavetables').makeTables(SR).forEach((t, id) => native.tableUpload(ctx, id, t))
  const prog = native.programBuild(ctx, uni.words, 0)
  const on = BigInt64Array.of(0n, 5n, -3n, 900n), thrown = []
  for (const args of [[prog, 4, 100, uni.params, null, 0, 4, 0, 1000, on, null], [prog, 4, 100, uni.params, null, 0, 0, 3, 1000, on, null],
    [prog, 4, 100, uni.params, new Float32Array(3), 0, 0, 0, 1000, on, null], [prog, 4, 100, uni.params, null, -1, 0, 0, 1000, on, null],
    [prog, 4, 100, null, null, 0, 0, 0, 1000, on, null], [prog, 4, 100, uni.params, null, 0, 0, 0, 1000], [prog, 4, 100, uni.params, null, 0, 0, 0, 0, on, null],
    [prog, 4, 100, uni.params, null, 0, 0, 0, 1000, [0, 1, 2, 3], null], [prog, 4, 100, uni.params, null, 0, 0, 0, 1000, BigInt64Array.of(0n, 1n, 2n), null],
    [prog, 4, 100, uni.params, null, 0, 0, 0, 1000, Float64Array.of(0, 1, 2.25, 3), null], [prog, 4, 100, uni.params, null, 0, 0, 0, 1000, on, new Float32Array(4)],
    [prog, 4, 100, uni.params, null, 0, 0, 0, 1000.5, on, null]])
    try { await native.renderScore(...args); thrown.push(null) } catch (e) { thrown.push(e) }
  note('addon rejections', thrown.every((e) => typeof e === 'string' && e.startsWith('dusp-hip:')), { thrown })
  note('addon rejections name the call', thrown.slice(0, 4).every((e) => typeof e === 'string' && e.startsWith('dusp-hip: renderScore:')) && !thrown.some((e) => /renderMix/.test(e)), { thrown })
  const direct = await native.renderScore(prog, 4, 100, uni.params, null, 3, 2, 0, 1000, on, BigInt64Array.of(100n, 0n, 50n, 100n))
  note('addon result', Buffer.isBuffer(direct.data) && direct.data.length === 1000 * 3 && direct.peaks instanceof Float32Array && direct.peaks.length === 1 && direct.peaks[0] > 0)
  const planar = await native.renderScore(prog, 4, 100, uni.params, null, 0, 0, 0, 1000, Float64Array.of(0, 5, -3, 900))
  note('addon planar result', planar instanceof Float32Array && planar.length === 1000 && planar.subarray(105, 900).every((v) => v === 0) && planar.subarray(900).some((v) => v !== 0))
  let stateRefused = null
  try { native.stateDownload(prog, 0, 0) } catch (e) { stateRefused = e }
  note('unit state after a score', typeof stateRefused === 'string' && stateRefused.includes('mix'), { stateRefused })
  native.programDestroy(prog)
  native.ctxDestroy(ctx)
  console.log(JSON.stringify(report))
}
main().catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack || e) })); process.exit(1) })
