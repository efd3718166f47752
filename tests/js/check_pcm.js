'use strict'
/* renderPcm / renderWav (GPU): frames encoded on the device against the host encoder (lib/wav.js) applied to the same
 * circuit's renderChannelData — byte for byte — the peak it reports, the host fall-back for event-segmented renders, and
 * the rejection strings.
 *   node check_pcm.js --sampleRate=48000 */
const lib = require('../../dusp_amd/js')
const SR = lib.config.sampleRate
const DUR = 0.05

const pan = () => new lib.Pan(new lib.Osc(440), 0.25)
const loud = () => new lib.Multiply(new lib.Osc(440), 3)
function evented() {
  const gain = new lib.Multiply(new lib.Osc(330), 1.5)
  gain.schedule(0.02, function () { this.B = 0.75 })
  return new lib.Multiply(gain, [1, 0.25])
}
const noisy = () => new lib.Multiply(new lib.Noise(), [0.5, 1.25]) // ticks on the host: arrives in f32 segments

function peakOf(cd) {
  let m = 0
  for (const ch of cd) for (const v of ch) m = Math.max(m, Math.abs(v))
  return m
}

async function main() {
  const report = { failed: [], checked: 0 }
  const note = (name, ok, extra) => { report.checked++; if (!ok) report.failed.push(Object.assign({ name }, extra)) }

  // a complete file from the device-encoded frames == the host encoder over the float render
  for (const bitDepth of [16, 24, 32]) {
    const file = await lib.renderWav(pan(), DUR, { bitDepth })
    const want = lib.encodeWav(await lib.renderChannelData(pan(), DUR), { bitDepth })
    note('renderWav ' + bitDepth, Buffer.isBuffer(file) && file.equals(want), { got: file.length, want: want.length })
    const back = lib.decodeWav(file)
    note('decode ' + bitDepth, back.numberOfChannels === 2 && back.bitDepth === bitDepth && back.sampleRate === SR && back.channelData[0].length === Math.trunc(DUR * SR))
  }

  // a circuit that clips, brought to full scale: the reported peak is the float render's maximum, the extreme sample +-full scale
  {
    const cd = await lib.renderChannelData(loud(), DUR), peak = peakOf(cd)
    for (const [bitDepth, full] of [[16, 32767], [24, 8388607]]) {
      const r = await lib.renderPcm(loud(), DUR, { bitDepth, normalise: 2 })
      let top = 0
      for (let p = 0; p < r.data.length; p += bitDepth / 8) top = Math.max(top, Math.abs(r.data.readIntLE(p, bitDepth / 8)))
      note('full scale ' + bitDepth, r.peak === peak && peak > 2.9 && top === full && r.numberOfChannels === 1 && r.bitDepth === bitDepth && r.sampleRate === SR,
        { peak: r.peak, want: peak, top })
      const host = lib.encodeFrames(Float32Array.from(cd[0]), 1, cd[0].length, bitDepth, 2)
      note('full scale bytes ' + bitDepth, r.data.equals(host.data) && host.peak === peak)
    }
    const clip = await lib.renderPcm(loud(), DUR, { bitDepth: 16, normalise: 1 }), full = await lib.renderPcm(loud(), DUR, { bitDepth: 16, normalise: 2 })
    note('clip == full when it clips', clip.data.equals(full.data))
    const quiet = await lib.renderPcm(pan(), DUR, { bitDepth: 16, normalise: 1 }), plain = await lib.renderPcm(pan(), DUR, { bitDepth: 16 })
    note('clip leaves what does not clip', quiet.data.equals(plain.data) && quiet.peak <= 1)
  }

  // segmented renders (a scheduled event; a host-ticked unit) take the host encoder: the same bytes as encoding renderChannelData's result
  {
    for (const bitDepth of [16, 24]) {
      const file = await lib.renderWav(evented(), DUR, { bitDepth, normalise: 2 })
      const cd = await lib.renderChannelData(evented(), DUR)
      const planar = new Float32Array(cd.length * cd[0].length)
      cd.forEach((ch, c) => planar.set(ch, c * cd[0].length))
      const host = lib.encodeFrames(planar, cd.length, cd[0].length, bitDepth, 2)
      const want = lib.encodeWav({ data: host.data, bitDepth, numberOfChannels: cd.length, sampleRate: SR })
      note('event fallback ' + bitDepth, file.equals(want) && cd.length === 2)
      const plain = await lib.renderWav(evented(), DUR, { bitDepth })
      note('event fallback, no gain ' + bitDepth, plain.equals(lib.encodeWav(cd, { bitDepth })))
    }
    const r = await lib.renderPcm(noisy(), DUR, { bitDepth: 16, normalise: 2 })
    let top = 0
    for (let p = 0; p < r.data.length; p += 2) top = Math.max(top, Math.abs(r.data.readInt16LE(p)))
    note('host-ticked unit', r.numberOfChannels === 2 && r.data.length === Math.trunc(DUR * SR) * 4 && top === 32767 && r.peak > 0 && r.peak <= 1.25)
  }

  // misuse rejects with strings
  const rejections = []
  for (const opts of [{ bitDepth: 8 }, { bitDepth: '16' }, { normalise: 3 }])
    await lib.renderPcm(pan(), DUR, opts).then(() => rejections.push(null), (e) => rejections.push(e))
  await lib.renderWav(pan(), DUR, { bitDepth: 12 }).then(() => rejections.push(null), (e) => rejections.push(e))
  note('rejections', rejections.every((e) => typeof e === 'string' && e.startsWith('dusp-hip:')), { rejections })
  // ... and so does the addon itself
  const native = require('../../dusp_amd/js/lib/native')()
  const ex = lib.extract(pan())
  const ctx = native.ctxCreate(-1)
  require('../../dusp_amd/js/lib/wavetables').makeTables(SR).forEach((t, id) => native.tableUpload(ctx, id, t))
  const prog = native.programBuild(ctx, ex.words, 0)
  const thrown = []
  for (const args of [[prog, 1, 100, null, 4, 0], [prog, 1, 100, null, 1, 5], [prog, 1, 100, null, 1]])
    try { await native.renderPcm(...args); thrown.push(null) } catch (e) { thrown.push(e) }
  note('addon rejections', thrown.every((e) => typeof e === 'string' && e.startsWith('dusp-hip:')), { thrown })
  const direct = await native.renderPcm(prog, 1, 1000, null, 2, 0)
  note('addon result', Buffer.isBuffer(direct.data) && direct.data.length === 1000 * 2 * 3 && direct.peaks instanceof Float32Array && direct.peaks.length === 1 && direct.peaks[0] > 0)
  native.programDestroy(prog)
  native.ctxDestroy(ctx)
  console.log(JSON.stringify(report))
}
main().catch((e) => { console.log(JSON.stringify({ fatal: String(e && e.stack || e) })); process.exit(1) })
