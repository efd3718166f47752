'use strict'
/* renderMix / renderMixPcm / renderMixWav (GPU): the mix of a batch, summed on the device in Sum.many's chain order, against the
 * Math.fround chain over renderMany's result — bit for bit — and, for voices the device renders bit for bit, against
 * renderChannelData(Sum.many(voices)); gains, a stereo voice, one voice, tiles, the encoded forms and the rejection strings.
 *   node check_mix.js --sampleRate=48000 */
const lib = require('../../dusp_amd/js')
const SR = lib.config.sampleRate
const DUR = 0.03

const VOICES = {
  osc: (k) => new lib.Osc(100.5 + 13 * k),
  fm: (k) => new lib.Multiply(new lib.Osc(new lib.Sum(new lib.Multiply(new lib.Osc(3 + k / 4), 40 + k), 220.5 + 10 * k)), new lib.Ramp(1200, 1, 0.25).trigger()),
  delay: (k) => new lib.Delay(new lib.Multiply(new lib.Osc(300 + 7 * k), 0.5 + k / 64), 100 + 20.5 * k, 4096),
  pan: (k) => new lib.Pan(new lib.Osc(200 + 7 * k), -0.9 + 0.05 * k), // two channels; pow() on the device: held to renderMany's own voices
  filtered: (k) => new lib.Filter(new lib.Osc(110 + 3.25 * k), 900 + 40 * k),
}
const EXACT = { osc: true, fm: true, delay: true, pan: false, filtered: false }
const voices = (kind, n) => Array.from({ length: n }, (_, k) => VOICES[kind](k))
const gainsFor = (n) => Float32Array.from({ length: n }, (_, k) => Math.fround(0.1 + 1.7 * ((k * 37) % 11) / 11))

/* the contract, in JavaScript: many[instance][channel] -> [channel] Float32Array */
function chain(many, gains) {
  const term = (i, c, t) => gains ? Math.fround(many[i][c][t] * gains[i]) : many[i][c][t]
  return many[0].map((ch, c) => {
    const out = new Float32Array(ch.length)
    for (let t = 0; t < ch.length; t++) {
      let acc = term(0, c, t)
      for (let i = 1; i < many.length; i++) acc = Math.fround(acc + term(i, c, t))
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
    for (const n of [1, 2, 37]) {
      const many = await lib.renderMany(voices(kind, n), DUR, { devices: [0] })
      const mix = await lib.renderMix(voices(kind, n), DUR)
      note(kind + ' x' + n + ' == chain over renderMany', mix.sampleRate === SR && mix.length === (kind === 'pan' ? 2 : 1) && sameBits(mix, chain(many)))
      const g = gainsFor(n)
      const mixG = await lib.renderMix(voices(kind, n), DUR, { gains: g, tileInstances: 5 })
      note(kind + ' x' + n + ' gains, tiles of 5', sameBits(mixG, chain(many, g)))
      if (EXACT[kind]) {
        const one = await lib.renderChannelData(lib.Sum.many(voices(kind, n)), DUR)
        note(kind + ' x' + n + ' == Sum.many', sameBits(mix, one))
        const oneG = await lib.renderChannelData(lib.Sum.many(voices(kind, n).map((v, k) => new lib.Multiply(v, g[k]))), DUR)
        note(kind + ' x' + n + ' gains == Sum.many of Multiply', sameBits(mixG, oneG))
      }
    }
  { // tiles and engines: the same bits
    const ref = await lib.renderMix(voices('delay', 37), DUR)
    for (const tileInstances of [1, 3, 64]) note('tile ' + tileInstances, sameBits(await lib.renderMix(voices('delay', 37), DUR, { tileInstances }), ref))
    note('chunk engine', sameBits(await lib.renderMix(voices('delay', 37), DUR, { engine: 1 }), ref))
    note('gains as a plain array', sameBits(await lib.renderMix(voices('fm', 9), DUR, { gains: Array.from(gainsFor(9)) }), await lib.renderMix(voices('fm', 9), DUR, { gains: gainsFor(9) })))
    note('no samples', (await lib.renderMix(voices('fm', 3), 0)).length === 0)
  }
  // the encoded forms: the host encoder over the f32 mix, and a file that decodes to the same frames
  for (const kind of ['pan', 'fm'])
    for (const bitDepth of [16, 24, 32]) {
      const mix = await lib.renderMix(voices(kind, 37), DUR)
      const planar = new Float32Array(mix.length * mix[0].length)
      mix.forEach((ch, c) => planar.set(ch, c * mix[0].length))
      const host = lib.encodeFrames(planar, mix.length, mix[0].length, bitDepth, 2)
      const pcm = await lib.renderMixPcm(voices(kind, 37), DUR, { bitDepth, normalise: 2 })
      note('renderMixPcm ' + kind + ' ' + bitDepth, pcm.data.equals(host.data) && pcm.peak === host.peak && pcm.peak > 1 && pcm.numberOfChannels === mix.length && pcm.bitDepth === bitDepth && pcm.sampleRate === SR,
        { peak: pcm.peak, want: host.peak })
      const file = await lib.renderMixWav(voices(kind, 37), DUR, { bitDepth })
      note('renderMixWav ' + kind + ' ' + bitDepth, file.equals(lib.encodeWav(mix, { bitDepth })))
      const back = lib.decodeWav(file), again = lib.decodeWav(lib.encodeWav(mix, { bitDepth }))
      note('renderMixWav decodes ' + kind + ' ' + bitDepth, back.numberOfChannels === mix.length && back.bitDepth === bitDepth && back.sampleRate === SR && sameBits(back.channelData, again.channelData) &&
        (bitDepth !== 32 || sameBits(back.channelData, mix)))
    }
  // what is refused, with strings
  const rejections = []
  const refused = (p) => p.then(() => rejections.push(null), (e) => rejections.push(e))
  await refused(lib.renderMix([new lib.Multiply(new lib.Noise(), 0.5), new lib.Multiply(new lib.Noise(), 0.25)], DUR)) // ticks on the host
  note('a Noise voice', typeof rejections[0] === 'string' && rejections[0].startsWith('dusp-hip: renderMix does not take circuits with host-ticked units'), { got: rejections[0] })
  const evented = (k) => { const v = new lib.Multiply(new lib.Osc(330 + k), 1.5); v.schedule(0.01, function () { this.B = 0.75 }); return v }
  await refused(lib.renderMix([evented(0), evented(1)], DUR))
  await refused(lib.renderMix(voices('fm', 3), DUR, { gains: [1, 2] }))
  await refused(lib.renderMix(voices('fm', 3), DUR, { tileInstances: 1.5 }))
  await refused(lib.renderMixPcm(voices('fm', 3), DUR, { bitDepth: 8 }))
  await refused(lib.renderMixWav(voices('fm', 3), DUR, { normalise: 3 }))
  note('rejections', rejections.length === 6 && rejections.every((e) => typeof e === 'string' && e.startsWith('dusp-hip:')), { rejections })
  // ... and the addon itself
  const native = require('../../dusp_amd/js/lib/native')()
  const uni = lib.unify(voices('fm', 4).map((v) => lib.extract(v)))
  const ctx = native.ctxCreate(-1)
  require('../../dusp_amd/js/lib/wavetables').makeTables(SR).forEach((t, id) => native.tableUpload(ctx, id, t))
  const prog = native.programBuild(ctx, uni.words, 0)
  const thrown = []
  for (const args of [[prog, 4, 100, uni.params, null, 0, 4, 0], [prog, 4, 100, uni.params, null, 0, 0, 3], [prog, 4, 100, uni.params, new Float32Array(3), 0, 0, 0],
    [prog, 4, 100, uni.params, null, -1, 0, 0], [prog, 4, 100, null, null, 0, 0, 0], [prog, 4, 100, uni.params, null, 0]])
    try { await native.renderMix(...args); thrown.push(null) } catch (e) { thrown.push(e) }
  note('addon rejections', thrown.every((e) => typeof e === 'string' && e.startsWith('dusp-hip:')), { thrown })
  const direct = await native.renderMix(prog, 4, 1000, uni.params, null, 3, 2, 0)
  note('addon result', Buffer.isBuffer(direct.data) && direct.data.length === 1000 * 3 && direct.peaks instanceof Float32Array && direct.peaks.length === 1 && direct.peaks[0] > 0)
  const planar = await native.renderMix(prog, 4, 1000, uni.params, null, 0, 0, 0)
  note('addon planar result', planar instanceof Float32Array && planar.length === 1000)
  let stateRefused = null
  try { native.stateDownload(prog, 0, 0) } catch (e) { stateRefused = e }
  note('unit state after a mix', typeof stateRefused === 'string' && stateRefused.includes('mix'), { stateRefused })
  native.programDestroy(prog)
  native.ctxDestroy(ctx)
  console.log(JSON.stringify(report))
}
main().catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack || e) })); process.exit(1) })
