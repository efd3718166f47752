'use strict'
/* renderChannelData(outlet | unit | patch, duration = 1, { TypedArray = Float32Array }) ->
 *   Promise<Array<TypedArray>> with `.sampleRate`
 * Drop-in for reference src/renderChannelData.js:5-49, executed on the MI355X through the N-API addon.
 * Misuse rejects with the reference's own strings; anything the GPU path cannot run rejects with a
 * "dusp-hip: ..." string (callers that hold the real `dusp` package can then fall back to it).
 *
 * After the render the circuit is consumed exactly as the reference leaves it: circuit.clock has
 * advanced by the ticked chunks and every unit's state fields (Osc.phase, Ramp.t/playing, Filter
 * history and coefficients, CircleBuffer node t, Timer.t, SampleRateRedux.val) hold the post-render values
 * (state write-back).
 */
const native = require('./native')
const config = require('./config')
const { extract, unify, deviceRetrigger } = require('./extract')
const { makeTables } = require('./wavetables')
const { OP, UNITS } = require('./ops')
const { MasterInput } = require('./graph')
const { encodeWav, encodeFrames } = require('./wav')

const contexts = new Map() // "sampleRate|device|slot" -> native context with that rate's wave tables

/* One context per (sample rate, device): a dusp_ctx is bound to one HIP device (include/dusp_hip.h "Threading").  device -1 = the
 * process's current device (single renders).  `slot` tells contexts of one device apart: renderMany's device list may name a GPU
 * twice (two contexts, two shards side by side on it). */
function contextFor(sampleRate, device = -1, slot = 0) {
  const key = sampleRate + '|' + device + '|' + slot
  if (!contexts.has(key)) {
    const n = native()
    const ctx = n.ctxCreate(device)
    makeTables(sampleRate).forEach((t, id) => n.tableUpload(ctx, id, t))
    contexts.set(key, ctx)
  }
  return contexts.get(key)
}

/* Contiguous, balanced split of n instances over `world` shards: the first n % world get one more (dusp_amd/shard.py
 * instance_range, SURVEY.md 8e: rank r renders [r N / G, (r + 1) N / G)). */
function instanceRange(n, rank, world) {
  const base = Math.floor(n / world), extra = n % world
  const lo = rank * base + Math.min(rank, extra)
  return [lo, lo + base + (rank < extra ? 1 : 0)]
}

/* The device list of a sharded render: undefined = every HIP device this process sees, a number n = devices 0 .. n-1, or the ids
 * themselves (one shard per entry, in order; an id may repeat). */
function deviceList(devices) {
  const n = native()
  const have = n.deviceCount()
  let list
  if (devices === undefined || devices === null) list = Array.from({ length: have }, (_, i) => i)
  else if (typeof devices === 'number') list = Array.from({ length: devices }, (_, i) => i)
  else list = Array.from(devices)
  if (!list.length) throw 'dusp-hip: renderMany: empty device list'
  for (const d of list)
    if (!Number.isInteger(d) || d < 0 || d >= have) throw 'dusp-hip: renderMany: device ' + d + ' is not one of the ' + have + ' this process sees'
  return list
}

function sampleCount(duration, sampleRate) {
  const n = Math.trunc(duration * sampleRate) // `new TypedArray(lengthInSamples)` truncates (:24,39)
  if (!(n >= 0)) throw 'dusp-hip: bad duration ' + duration
  return n
}

function writeBack(n, prog, circuit, chunkSize, nSamples) {
  circuit.units.forEach((unit, u) => {
    if (deviceRetrigger(unit, circuit.units)) { unit.t = n.stateDownload(prog, 0, u)[0]; return }
    const spec = UNITS[unit.constructor.name]
    if (!spec) return
    if (spec.op === OP.OSC) unit.phase = n.stateDownload(prog, 0, u)[0]
    else if (spec.op === OP.RAMP) { const s = n.stateDownload(prog, 0, u); unit.t = s[0]; unit.playing = s[1] !== 0 }
    else if (spec.op === OP.CB_READER || spec.op === OP.CB_WRITER) unit.t = n.stateDownload(prog, 0, u)[0]
    else if (spec.op === OP.FIXED_DELAY || spec.op === OP.COMB_FILTER || spec.op === OP.ALL_PASS || spec.op === OP.READBACK_DELAY)
      unit.tBuffer = n.stateDownload(prog, 0, u)[0]
    else if (spec.op === OP.TIMER) unit.t = n.stateDownload(prog, 0, u)[0]
    else if (spec.op === OP.SHAPE) {
      const s = n.stateDownload(prog, 0, u)
      const finishedNow = s[2] !== 0 && !unit.finished
      unit.t = s[0]; unit.playing = s[1] !== 0; unit.finished = s[2] !== 0
      if (finishedNow && unit.onFinish) unit.onFinish() // hostOnly hooks only (the extractor refuses the rest)
    } else if (spec.op === OP.AHD) {
      const s = n.stateDownload(prog, 0, u)
      unit.state = s[0]; unit.playing = s[1] !== 0; unit.t = s[2]
    }
    else if (spec.op === OP.SAMPLE_RATE_REDUX) {
      const s = n.stateDownload(prog, 0, u)
      unit.timeSinceLastUpdate = s[0]
      unit.val = Array.from(s.subarray ? s.subarray(2, 2 + s[1]) : s.slice(2, 2 + s[1]))
    } else if (spec.op === OP.MULTI_OSC) { const s = n.stateDownload(prog, 0, u); for (let c = 0; c < s[0]; c++) unit.phase[c] = s[1 + c] }
    else if (spec.op === OP.FILTER) {
      const s = n.stateDownload(prog, 0, u)
      if (s[0]) unit.lastF = s[1]
      unit.a0 = s[2]; unit.a1 = s[3]; unit.a2 = s[4]; unit.b1 = s[5]; unit.b2 = s[6]
      for (let c = 0; c < s[7]; c++) {
        unit.x1[c] = s[8 + 4 * c]; unit.x2[c] = s[9 + 4 * c]; unit.y1[c] = s[10 + 4 * c]; unit.y2[c] = s[11 + 4 * c]
      }
    }
  })
  circuit.clock += Math.ceil(nSamples / chunkSize) * chunkSize
}

const RESUMABLE = 0x100 // DUSP_ENGINE_RESUMABLE (include/dusp_hip.h)

/* A circuit's wiring by unit identity, in process order: which units, and what feeds every inlet.  A host callback that
 * rewires the graph (`a then b`, constructOperation.js:45-61: the finish hook of `a` points a Repeater at `b`, whose units join
 * the running circuit) shows up as another text; the device program is then built again for the new circuit, every unit's
 * state coming from the objects (the state write-back of the segment before). */
const unitIds = new WeakMap()
let nextUnitId = 1
const idOf = (u) => { if (!unitIds.has(u)) unitIds.set(u, nextUnitId++); return unitIds.get(u) }
const RING_OPS = new Set([OP.DELAY, OP.MONO_DELAY, OP.READBACK_DELAY, OP.FIXED_DELAY, OP.COMB_FILTER, OP.ALL_PASS, OP.CB_READER, OP.CB_WRITER])
function wiringOf(circuit) {
  const units = circuit.units
  const at = new Map(units.map((u, i) => [u, i]))
  const ids = new Set(), late = [] // late: edges read a chunk late (the source ticks after its reader), as [source id, reader id]
  let text = '', rings = false
  units.forEach((u, i) => {
    ids.add(idOf(u))
    const spec = UNITS[u.constructor.name]
    if (spec && RING_OPS.has(spec.op)) rings = true
    text += idOf(u) + '('
    for (const name of Object.keys(u.inlets || {})) {
      const inlet = u.inlets[name]
      if (inlet.connected) {
        const src = inlet.outlet.unit
        text += name + ':' + idOf(src) + ','
        if (!(at.get(src) < i)) late.push([idOf(src), idOf(u)])
      }
    }
    text += ')'
  })
  return { text, ids, late, rings }
}
/* Why a rewired circuit cannot simply start on a new device program (null: it can).  What a program keeps on the device only
 * — delay lines, CircleBuffers, the previous chunk of an outlet that something reads a chunk late — would have to move into the
 * new program's layout; not built, so such circuits are refused rather than rendered from zeros. */
function cannotRebuild(before, after) {
  if (before.rings) return 'the circuit holds delay lines or CircleBuffers on the device'
  if (before.late.length) return 'an edge of the circuit is read a chunk late, its last chunk lives on the device'
  for (const [src] of after.late) if (before.ids.has(src)) return 'the new process order reads a unit of the old circuit a chunk late'
  return null
}

/* Renders a circuit piecewise, in time order.  Every call continues where the previous one stopped:
 *
 * Event-segmented rendering (SURVEY.md 8f-3).  The reference runs every event with t < clock + chunk at the start
 * of the tick at `clock` (Circuit.js:23,57-65), i.e. events take effect on chunk boundaries.  So: run the due
 * callbacks on the host objects, render up to the chunk in which the next event falls due, write the unit state
 * back, re-extract and CONTINUE the same device program (dusp_program_continue: unit state and constants come from
 * the objects, delay lines / CircleBuffers / feedback chunks stay resident on the device). */
class SegmentRenderer {
  constructor(outlet, { engine = 0, resumable = false } = {}) {
    this.outlet = outlet
    this.first = extract(outlet, { allowEvents: true })
    this.circuit = this.first.circuit
    this.chunk = this.first.chunkSize
    this.sampleRate = this.first.sampleRate
    this.retick()
    this.hasEvents = !!(this.circuit.events && this.circuit.events.length) || this.tickers.length > 0
    this.engine = resumable || this.hasEvents ? engine | RESUMABLE : engine
    this.native = native()
    this.prog = null
    this.wiring = null
    this.clock = 0
  }

  // units that act through host callbacks between chunks (Retriggerer, SporadicRetriggerer; host-computed signals: Noise): ticked here, firing = segment boundary
  retick() {
    this.tickers = this.circuit.units.filter((u) => ((UNITS[u.constructor.name] && UNITS[u.constructor.name].hostTick) || u.isHostSignal) &&
      !deviceRetrigger(u, this.circuit.units)) // (a Retriggerer of a Shape / AHD runs on the device)
    for (const u of this.tickers)
      if (!u.hostTick) throw 'dusp-hip: ' + u.label + ' needs host-side ticking, which only this package\'s own unit classes provide'
  }

  /* the next nSamples samples (a whole number of chunks, except in the last call of a render) ->
   * { pcm: Float32Array [channel][nSamples], nChannels } */
  async next(nSamples) {
    const n = this.native, chunk = this.chunk
    const start = this.clock
    const end = start + Math.ceil(nSamples / chunk) * chunk
    const pieces = []
    while (this.clock < end) {
      let next = end
      if (this.circuit.events && this.circuit.events.length) {
        this.circuit.runEvents(this.clock + chunk)
        if (this.circuit.events.length) {
          const due = Math.floor(this.circuit.events[0].t / chunk) * chunk
          next = Math.min(end, Math.max(this.clock + chunk, due))
        }
      }
      if (this.tickers.length) { // this chunk's host ticks (after the events, as in Circuit.tick), then run up to the next firing
        for (const u of this.tickers) u.hostTick(chunk)
        // look ahead chunk by chunk, every ticker in tick order (the random ones draw their numbers in the reference's
        // order), never past the next scheduled event; the first chunk in which anything fires starts the next segment
        const room = (next - this.clock) / chunk - 1
        let quiet = 0
        for (const u of this.tickers) u.peekBegin()
        while (quiet < room) {
          let fires = false
          for (const u of this.tickers) fires = u.peekNext(chunk) || fires
          if (fires) break
          quiet++
        }
        for (const u of this.tickers) u.skipQuiet(chunk, quiet)
        next = this.clock + (1 + quiet) * chunk
      }
      const ex = !this.prog && !this.hasEvents ? this.first : extract(this.outlet, { allowEvents: true, allowClock: true })
      const wiring = wiringOf(ex.circuit)
      if (this.prog && wiring.text !== this.wiring.text) { // a callback rewired the circuit (`then`: unDusp.js): another device program from here on
        const why = cannotRebuild(this.wiring, wiring)
        if (why) throw 'dusp-hip: the circuit was rewired during the render (' + why + '): not supported on the GPU path'
        n.programDestroy(this.prog)
        this.prog = null
        this.circuit = ex.circuit
        const before = this.tickers
        this.retick()
        if (this.tickers.length !== before.length || this.tickers.some((u, i) => u !== before[i]))
          throw 'dusp-hip: the circuit was rewired during the render (units that tick on the host joined or left): not supported on the GPU path'
      }
      this.wiring = wiring
      if (!this.prog) this.prog = n.programBuild(contextFor(ex.sampleRate), ex.words, this.engine)
      else n.programContinue(this.prog, ex.words)
      const len = Math.min(next, start + nSamples) - this.clock // the last segment may end inside a chunk
      let inputs = null // the host-computed signals of this segment: [source][len]
      if (ex.sources.length) {
        inputs = new Float32Array(ex.sources.length * len)
        ex.sources.forEach((u, k) => u.takeSegment(len, inputs, k * len))
      }
      // Float32Array [channel][len]; or, for renderPcm's single segment, { data: Buffer of encoded frames, peaks }
      const pcm = this.encode ? await n.renderPcm(this.prog, 1, len, null, this.encode.format, this.encode.normalise, inputs)
        : await n.render(this.prog, 1, len, null, false, inputs)
      writeBack(n, this.prog, this.circuit, chunk, len) // advances circuit.clock to `next`
      pieces.push({ pcm, len, nChannels: n.programInfo(this.prog).nOutChannels })
      this.clock = next
    }
    const nChannels = Math.max(...pieces.map((p) => p.nChannels))
    if (pieces.length === 1) return { pcm: pieces[0].pcm, nChannels }
    const pcm = new Float32Array(nChannels * nSamples) // late channels start as zeros (renderChannelData.js:38-39)
    let at = 0
    for (const p of pieces) {
      for (let c = 0; c < p.nChannels; c++) pcm.set(p.pcm.subarray(c * p.len, (c + 1) * p.len), c * nSamples + at)
      at += p.len
    }
    return { pcm, nChannels }
  }

  close() {
    if (this.prog) this.native.programDestroy(this.prog)
    this.prog = null
  }
}

async function renderChannelData(outlet, duration = 1, { TypedArray = Float32Array, engine = 0 } = {}) {
  const renderer = new SegmentRenderer(outlet, { engine })
  try {
    const nSamples = sampleCount(duration, renderer.sampleRate)
    const channelData = []
    channelData.sampleRate = renderer.sampleRate
    if (nSamples === 0) return channelData
    const { pcm, nChannels } = await renderer.next(nSamples)
    for (let c = 0; c < nChannels; c++) {
      const channel = pcm.subarray(c * nSamples, (c + 1) * nSamples) // Float32Array: handed over without a copy
      channelData.push(TypedArray === Float32Array ? channel : TypedArray.from(channel))
    }
    return channelData
  } finally {
    renderer.close()
  }
}

const PCM_FORMAT = { 16: 1, 24: 2, 32: 3 } // DUSP_PCM_S16 / _S24 / _F32 (include/dusp_hip.h)

/* renderChannelData, delivering peak-normalised frames: resolves to { data: Buffer, bitDepth, numberOfChannels, sampleRate, peak }
 * — data holds interleaved little-endian int16 / packed int24 (or f32 at bitDepth 32), peak the render's max |x| before the gain;
 * normalise 0: none, 1: shrink only a render that would clip, 2: to full scale (one gain for all channels; the sample contract is in
 * include/dusp_hip.h, "Device-side PCM delivery").
 *
 * A circuit without scheduled events and host-ticked units is ONE device render: the peak search, the gain, the quantisation and the
 * interleave run on the GPU (dusp_render_host_pcm) and 2 or 3 bytes per sample are downloaded.  A circuit that is rendered in segments
 * arrives as f32 on the host and is encoded here by the same contract (wav.js encodeFrames), the peak taken over the whole render.
 * The bytes are the same either way. */
async function renderPcm(outlet, duration = 1, { bitDepth = 16, normalise = 0, engine = 0 } = {}) {
  if (bitDepth !== 16 && bitDepth !== 24 && bitDepth !== 32) throw 'dusp-hip: renderPcm: bitDepth must be 16, 24 or 32' // (numbers: '16' is refused like 8)
  if (normalise !== 0 && normalise !== 1 && normalise !== 2) throw 'dusp-hip: renderPcm: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale)'
  const renderer = new SegmentRenderer(outlet, { engine })
  try {
    const sampleRate = renderer.sampleRate, nSamples = sampleCount(duration, sampleRate)
    if (nSamples === 0) return { data: Buffer.alloc(0), bitDepth, numberOfChannels: 0, sampleRate, peak: 0 }
    if (!renderer.hasEvents) renderer.encode = { format: PCM_FORMAT[bitDepth], normalise }
    const { pcm, nChannels } = await renderer.next(nSamples)
    if (renderer.encode) return { data: pcm.data, bitDepth, numberOfChannels: nChannels, sampleRate, peak: pcm.peaks[0] }
    const { data, peak } = encodeFrames(pcm, nChannels, nSamples, bitDepth, normalise)
    return { data, bitDepth, numberOfChannels: nChannels, sampleRate, peak }
  } finally {
    renderer.close()
  }
}

/* renderPcm plus the RIFF/WAVE header: resolves to a Buffer holding a complete file. */
async function renderWav(outlet, duration = 1, opts = {}) {
  return encodeWav(await renderPcm(outlet, duration, opts))
}

/* The circuits of a batch render as ONE program: extracted (scheduled events are refused there) and unified.  One launch for all
 * circuits: nothing ticks on the host in between, so units that need that are refused, not ignored. */
function unifyBatch(outlets, who) {
  const extractions = outlets.map((o) => extract(o))
  for (const ex of extractions)
    for (const u of ex.circuit.units)
      if ((u.isHostSignal || (UNITS[u.constructor.name] && UNITS[u.constructor.name].hostTick)) && !deviceRetrigger(u, ex.circuit.units))
        throw 'dusp-hip: ' + who + ' does not take circuits with host-ticked units (' + u.label + '): render them one by one'
  return unify(extractions)
}

/* N structurally identical circuits (voices, a parameter sweep) as ONE GPU program per device:
 * resolves to result[instance][channel] = Float32Array(duration * sampleRate).
 *
 * The instances share nothing, so they shard over the GPUs of the node with no exchange at all (SURVEY.md 8e): `devices` (default:
 * every HIP device the process sees; a count; or a list of ids) names one shard per entry, shard r renders the contiguous instance
 * range instanceRange(N, r, shards) on a context of ITS device — the same program text, its rows of the parameter table — and all
 * shards are in flight at once (one async render each on the libuv pool; the addon serialises calls per context, not across them).
 * The results come back in instance order whatever order the devices finish in.  A render rejects as a whole with the first
 * failing shard's string. */
async function renderMany(outlets, duration = 1, { engine = 0, devices } = {}) {
  const uni = unifyBatch(outlets, 'renderMany')
  const nSamples = sampleCount(duration, uni.sampleRate)
  if (nSamples === 0) return outlets.map(() => [])
  const n = native()
  const list = deviceList(devices)
  const seen = new Map() // device id -> contexts of it handed out so far
  const shards = []
  for (let r = 0; r < list.length; r++) {
    const [lo, hi] = instanceRange(uni.nInstances, r, list.length)
    if (hi === lo) continue
    const slot = seen.get(list[r]) || 0
    seen.set(list[r], slot + 1)
    shards.push({ lo, hi, device: list[r], slot, prog: null })
  }
  try {
    for (const sh of shards) sh.prog = n.programBuild(contextFor(uni.sampleRate, list.length === 1 && devices === undefined ? -1 : sh.device, sh.slot), uni.words, engine)
    const jobs = shards.map((sh) => {
      let params = null
      if (uni.nParams) { // slot-major [nParams][nInstances]: this shard's columns of every row
        const count = sh.hi - sh.lo
        params = new Float32Array(uni.nParams * count)
        for (let p = 0; p < uni.nParams; p++) params.set(uni.params.subarray(p * uni.nInstances + sh.lo, p * uni.nInstances + sh.hi), p * count)
      }
      return n.render(sh.prog, sh.hi - sh.lo, nSamples, params)
    })
    const pcms = await Promise.all(jobs.map((j) => j.then((v) => ({ ok: v }), (e) => ({ err: e })))) // (every shard ends before anything is torn down)
    const failed = pcms.find((p) => p.err !== undefined)
    if (failed) throw failed.err
    const result = new Array(uni.nInstances)
    shards.forEach((sh, k) => {
      const nCh = n.programInfo(sh.prog).nOutChannels, pcm = pcms[k].ok
      for (let i = sh.lo; i < sh.hi; i++) {
        const chans = []
        for (let c = 0; c < nCh; c++) {
          const at = ((i - sh.lo) * nCh + c) * nSamples
          chans.push(pcm.subarray(at, at + nSamples))
        }
        chans.sampleRate = uni.sampleRate
        result[i] = chans
      }
    })
    return result
  } finally {
    for (const sh of shards) if (sh.prog) n.programDestroy(sh.prog)
  }
}

/* The MIX of N structurally identical circuits — what renderChannelData(Sum.many(outlets), duration) computes: the reference's
 * left-deep chain ((v0 + v1) + v2) + ..., one f32 rounding per add (Sum.js:18-29), with `gains` the chain over Multiply(outlet, g_i) —
 * rendered as ONE program, tile by tile, and summed ON THE DEVICE in that order (dusp_render_host_mix).  Device memory is bounded
 * by the tile (tileInstances; 0: the library's default), not by N, and one voice's worth of samples is downloaded, where renderMany
 * downloads every voice.  One device.  A voice sample that is NaN drops that voice out of the sample (the reference's Sum would zero
 * the mix sample there).  Resolves to channelData like renderChannelData; circuits with scheduled events or host-ticked units are
 * refused as renderMany refuses them. */
async function mixCall(who, outlets, duration, opts, format, normalise, score = false) {
  const { gains, engine = 0, tileInstances = 0 } = opts
  const uni = unifyBatch(outlets, who)
  const nSamples = sampleCount(duration, uni.sampleRate) // (of a score: the timeline's)
  let nVoiceSamples = 0, onsets = null, lengths = null
  if (score) {
    nVoiceSamples = sampleCount(opts.voiceDuration === undefined ? 1 : opts.voiceDuration, uni.sampleRate)
    if (nVoiceSamples === 0) throw 'dusp-hip: ' + who + ': voiceDuration must cover at least one sample'
    onsets = wholeSamples(who, 'onsets', opts.onsets, uni.nInstances)
    if (opts.lengths !== undefined && opts.lengths !== null) lengths = wholeSamples(who, 'lengths', opts.lengths, uni.nInstances)
  }
  let g = null
  if (gains !== undefined && gains !== null) {
    g = gains instanceof Float32Array ? gains : Float32Array.from(gains)
    if (g.length !== uni.nInstances) throw 'dusp-hip: ' + who + ': gains must hold one value per outlet'
  }
  if (!Number.isInteger(tileInstances) || tileInstances < 0) throw 'dusp-hip: ' + who + ': tileInstances must be 0 (the default tile) or a whole number of instances'
  const n = native()
  const prog = n.programBuild(contextFor(uni.sampleRate), uni.words, engine)
  try {
    const nChannels = n.programInfo(prog).nOutChannels
    if (nSamples === 0) return { nSamples, nChannels, sampleRate: uni.sampleRate, result: null }
    const params = uni.nParams ? uni.params : null
    const result = score
      ? await n.renderScore(prog, uni.nInstances, nVoiceSamples, params, g, tileInstances, format, normalise, nSamples, onsets, lengths)
      : await n.renderMix(prog, uni.nInstances, nSamples, params, g, tileInstances, format, normalise)
    return { nSamples, nChannels, sampleRate: uni.sampleRate, result }
  } finally {
    n.programDestroy(prog)
  }
}

async function renderMix(outlets, duration = 1, opts = {}) {
  const { nSamples, nChannels, sampleRate, result } = await mixCall('renderMix', outlets, duration, opts, 0, 0)
  const channelData = []
  channelData.sampleRate = sampleRate
  if (result) for (let c = 0; c < nChannels; c++) channelData.push(result.subarray(c * nSamples, (c + 1) * nSamples))
  return channelData
}

/* renderMix, delivering what renderPcm delivers: the mix's frames, encoded on the device, and the mix's peak. */
async function renderMixPcm(outlets, duration = 1, opts = {}) {
  const { bitDepth = 16, normalise = 0 } = opts
  if (bitDepth !== 16 && bitDepth !== 24 && bitDepth !== 32) throw 'dusp-hip: renderMixPcm: bitDepth must be 16, 24 or 32'
  if (normalise !== 0 && normalise !== 1 && normalise !== 2) throw 'dusp-hip: renderMixPcm: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale)'
  const { nChannels, sampleRate, result } = await mixCall('renderMixPcm', outlets, duration, opts, PCM_FORMAT[bitDepth], normalise)
  if (!result) return { data: Buffer.alloc(0), bitDepth, numberOfChannels: 0, sampleRate, peak: 0 }
  return { data: result.data, bitDepth, numberOfChannels: nChannels, sampleRate, peak: result.peaks[0] }
}

async function renderMixWav(outlets, duration = 1, opts = {}) {
  return encodeWav(await renderMixPcm(outlets, duration, opts))
}

/* onsets / lengths of a score, one per outlet, in SAMPLES: a BigInt64Array, a Float64Array or an array of whole numbers (the addon
 * refuses a fraction) */
function wholeSamples(who, name, values, count) {
  let a = values
  if (Array.isArray(a)) a = a.length && typeof a[0] === 'bigint' ? BigInt64Array.from(a) : Float64Array.from(a)
  if (!(a instanceof BigInt64Array) && !(a instanceof Float64Array)) throw 'dusp-hip: ' + who + ': ' + name + ' must be a BigInt64Array, a Float64Array or an array of whole numbers (in samples)'
  if (a.length !== count) throw 'dusp-hip: ' + who + ': ' + name + ' must hold one value per outlet'
  if (a instanceof Float64Array && !a.every(Number.isInteger)) throw 'dusp-hip: ' + who + ': ' + name + ' are in samples, whole numbers: a fraction is refused'
  return a
}

/* A PIECE of N structurally identical circuits: voice k starts at sample onsets[k] of a timeline of `duration` seconds — what
 * renderChannelData(Sum.many(outlets.map((v, k) => new Delay(v, onsets[k], maxDelay))), duration) computes (a Delay by whole samples
 * is its input behind zeros; the voice with onset 0 bare) — rendered as ONE program for `voiceDuration` seconds a voice, tile by tile,
 * and mixed ON THE DEVICE at the onsets in Sum.many's chain order (dusp_render_host_score).  onsets and lengths are in samples, whole
 * numbers of any sign (a negative onset: the voice began before the timeline; lengths clip a voice to its first samples); the
 * durations are in seconds.  gains, engine, tileInstances and the refusals are renderMix's.  pans: as renderPiece's — mono voices, two
 * channels out, through the piece's call with the score as its one part (voiceDuration is one number; tileInstances does not apply).
 * fracs: as renderPiece's — voice k starts at onsets[k] + fracs[k] samples — through the piece's call too.
 * places (with speakers, decibelsPerMetre, sampleDelayPerMetre): as renderPiece's — mono voices, one channel a speaker — through the
 * piece's call too.
 * stereo: true — as renderPiece's: voices of one or two channels, two channels out, pans optional and null / NaN for a voice that is not
 * placed — through the piece's call too.
 * master: as renderPiece's — the mix through a mono circuit, channel by channel, on the device — through the piece's call too.
 * buses, sends: as renderPiece's — per-voice send levels into effect buses beside the mix — through the piece's call too.
 * stems: true — as renderPiece's: the direct mix, every track and every bus return beside the mix — through the piece's call too.
 * meters: true — as renderPiece's: the RMS and the BS.1770 loudness of every signal the call delivers — through the piece's call too.
 * truePeak: true, and on the Pcm / Wav forms loudness, truePeakMax, limiter, limiterWindow, limiterRelease — as renderPiece's — through the piece's call too. */
const given = (x) => x !== undefined && x !== null
const asPiece = (opts) => given(opts.pans) || given(opts.fracs) || given(opts.places) || opts.stereo === true || given(opts.master) || given(opts.buses) || given(opts.sends) ||
  given(opts.tracks) || given(opts.trackOf) || given(opts.faders) || given(opts.trackSends) || (opts.stems !== undefined && opts.stems !== false) ||
  (opts.meters !== undefined && opts.meters !== false) || (opts.truePeak !== undefined && opts.truePeak !== false) || given(opts.loudness) || (opts.limiter !== undefined && opts.limiter !== false) || given(opts.limiterRelease)

function scoreAsPiece(opts) { // renderScore with pans, fracs or places: the piece's call with the score as its one part
  return Object.assign({}, opts, { voiceDurations: opts.voiceDuration === undefined ? 1 : opts.voiceDuration, tileBytes: 0 })
}

async function renderScore(outlets, opts = {}) {
  const { duration = 1 } = opts
  const { nSamples, nChannels, sampleRate, result, names, metered } = asPiece(opts)
    ? await pieceCall('renderScore', outlets, scoreAsPiece(opts), 0, 0, true)
    : await mixCall('renderScore', outlets, duration, opts, 0, 0, true)
  if (names) return withMeters(planarStems(names, nSamples, nChannels, sampleRate, result), metered)
  const channelData = []
  channelData.sampleRate = sampleRate
  if (result) for (let c = 0; c < nChannels; c++) channelData.push(result.subarray(c * nSamples, (c + 1) * nSamples))
  return withMeters(channelData, metered)
}

async function renderScorePcm(outlets, opts = {}) {
  const { duration = 1, bitDepth = 16, normalise = 0 } = opts
  if (bitDepth !== 16 && bitDepth !== 24 && bitDepth !== 32) throw 'dusp-hip: renderScorePcm: bitDepth must be 16, 24 or 32'
  if (normalise !== 0 && normalise !== 1 && normalise !== 2) throw 'dusp-hip: renderScorePcm: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale)'
  const { nChannels, sampleRate, result, names, metered, loud } = asPiece(opts)
    ? await pieceCall('renderScorePcm', outlets, scoreAsPiece(opts), PCM_FORMAT[bitDepth], normalise, true)
    : await mixCall('renderScorePcm', outlets, duration, opts, PCM_FORMAT[bitDepth], normalise, true)
  if (names) return withMeters(pcmStems(names, nChannels, sampleRate, result, bitDepth, normalise), metered, loud)
  if (!result) return withMeters({ data: Buffer.alloc(0), bitDepth, numberOfChannels: 0, sampleRate, peak: 0 }, metered, loud)
  return withMeters({ data: result.data, bitDepth, numberOfChannels: nChannels, sampleRate, peak: result.peaks[0] }, metered, loud)
}

async function renderScoreWav(outlets, opts = {}) {
  return wavOf(await renderScorePcm(outlets, opts))
}

/* What two extractions have in common exactly when unify takes them as instances of one program: the descriptor's words with the
 * values at the constant sites masked (twin of render.py structure_key). */
function structureKey(extraction) {
  const words = Float64Array.from(extraction.words)
  for (const s of extraction.constSites) for (let k = 0; k < s.n; k++) words[s.valPos + k] = 0
  return Buffer.from(words.buffer, words.byteOffset, words.byteLength).toString('latin1')
}

/* Group the voices of a piece into parts by structure and by voiceSamples[k]; parts are numbered in the order their first voice comes
 * in the list.  Needs no device.  -> { parts: [{ uni, nVoiceSamples }], partOf: Uint32Array, instanceOf: [], sampleRate } — voice k is
 * instance instanceOf[k] of part partOf[k], which is also the next unused instance of that part (twin of render.py piece_parts). */
function pieceParts(extractions, voiceSamples) {
  if (extractions.length === 0) throw 'dusp-hip: no instances'
  const rates = [...new Set(extractions.map((e) => e.sampleRate))]
  if (rates.length !== 1) throw 'dusp-hip: the voices of a piece have one sample rate, not ' + rates.sort()
  const index = new Map(), members = [], samples = [], partOf = new Uint32Array(extractions.length), instanceOf = []
  extractions.forEach((e, k) => {
    const key = voiceSamples[k] + ':' + structureKey(e)
    if (!index.has(key)) {
      index.set(key, members.length)
      members.push([])
      samples.push(voiceSamples[k])
    }
    const p = index.get(key)
    partOf[k] = p
    instanceOf.push(members[p].length)
    members[p].push(e)
  })
  return { parts: members.map((m, p) => ({ uni: unify(m), nVoiceSamples: samples[p] })), partOf, instanceOf, sampleRate: rates[0] }
}

/* channels[p]: the output channels of part p's circuit.  A piece has one channel count: refused by string otherwise. */
function checkPieceChannels(channels) {
  channels.forEach((c, p) => {
    if (c !== channels[0]) throw 'dusp-hip: the voices of a piece must have one number of output channels: part ' + p + ' has ' + c + ', part 0 has ' + channels[0]
  })
  return channels[0]
}

/* channels[p]: the output channels of part p's circuit.  A panned voice is mono: refused by string otherwise (twin of render.py
 * check_pan_channels). */
function checkPanChannels(channels) {
  channels.forEach((c, p) => {
    if (c !== 1) throw 'dusp-hip: a panned voice is mono: part ' + p + ' has ' + c + ' output channels'
  })
  return 2
}

/* pans of `count` voices -> { pans: Float32Array, comp: Float64Array }: checked — one finite pan a voice, not clamped — with the
 * reference Pan unit's compensation 10^((1 - |pan|) * 1.5 / 20) by Math.pow, as Pan.js computes it (twin of runtime.py pan_arrays). */
function panArrays(pans, count) {
  const ok = Array.isArray(pans) || pans instanceof Float32Array || pans instanceof Float64Array
  const p = ok ? (pans instanceof Float32Array ? pans : Float32Array.from(pans)) : null
  if (!p || p.length !== count) throw 'dusp-hip: pans must have shape (voices=' + count + ',)'
  for (let k = 0; k < count; k++) if (!Number.isFinite(p[k])) throw 'dusp-hip: the pan of voice ' + k + ' is not finite'
  return { pans: p, comp: Float64Array.from(p, (x) => Math.pow(10, ((1 - Math.abs(x)) * 1.5) / 20)) }
}

/* pans of `count` voices of a stereo piece -> { pans: Float32Array with NaN for "not placed", comp: Float64Array }: undefined / null
 * (nothing placed) or one entry a voice, a number, null or NaN; an infinite pan is refused (twin of runtime.py stereo_pan_arrays).  The
 * compensation is panArrays'; an unplaced voice's is 1 and is not read. */
function stereoPanArrays(pans, count) {
  if (!given(pans)) pans = new Float32Array(count).fill(NaN)
  const ok = Array.isArray(pans) || pans instanceof Float32Array || pans instanceof Float64Array
  const p = ok ? (pans instanceof Float32Array ? pans : Float32Array.from(pans, (x) => (x === null ? NaN : x))) : null
  if (!p || p.length !== count) throw 'dusp-hip: pans must have shape (voices=' + count + ',)'
  for (let k = 0; k < count; k++) if (p[k] === Infinity || p[k] === -Infinity) throw 'dusp-hip: the pan of voice ' + k + ' is not finite'
  return { pans: p, comp: Float64Array.from(p, (x) => (Number.isNaN(x) ? 1 : Math.pow(10, ((1 - Math.abs(x)) * 1.5) / 20))) }
}

/* channels[k]: the channels of voice k, pans: stereoPanArrays'.  A voice of a stereo piece is mono or has two channels, and only a mono
 * voice is placed: refused by string otherwise (twin of mix.py check_stereo_kinds). */
function checkStereoKinds(channels, pans) {
  channels.forEach((c, k) => {
    if (c !== 1 && c !== 2) throw 'dusp-hip: a voice of a stereo piece has one or two channels: voice ' + k + ' has ' + c
    if (c === 2 && !Number.isNaN(pans[k])) throw 'dusp-hip: a two-channel voice is not panned: the pan of voice ' + k + ' must be NaN (not placed)'
  })
  return 2
}

const STEREO_NO_PLACES = 'dusp-hip: places and stereo do not go together: a placed voice is mono and the speakers are the channels'

/* fracs of `count` voices -> Float64Array: checked — one finite fraction of a sample a voice, 0 <= f < 1 — by the strings the library
 * uses (twin of mix.py check_fracs). */
function fracArrays(fracs, count) {
  const ok = Array.isArray(fracs) || fracs instanceof Float32Array || fracs instanceof Float64Array
  const f = ok ? (fracs instanceof Float64Array ? fracs : Float64Array.from(fracs)) : null
  if (!f || f.length !== count) throw 'dusp-hip: fracs must have shape (voices=' + count + ',)'
  for (let k = 0; k < count; k++) if (!Number.isFinite(f[k])) throw 'dusp-hip: the fraction of voice ' + k + ' is not finite'
  for (let k = 0; k < count; k++) if (f[k] < 0 || f[k] >= 1) throw 'dusp-hip: the fraction of voice ' + k + ' is outside [0, 1)'
  return f
}

/* Positions on the timeline in samples, real numbers of any sign -> { onsets: Float64Array of whole numbers, fracs: Float64Array } by
 * floor: position = onset + frac with 0 <= frac < 1, what the `onsets` and `fracs` options take.  A negative position so close to a whole
 * number that position - floor(position) rounds to 1 is that whole number (twin of mix.py split_onsets). */
function splitOnsets(positions) {
  const p = Float64Array.from(positions)
  if (!p.every(Number.isFinite) || p.some((x) => x >= 2 ** 63 || x < -(2 ** 63))) throw 'dusp-hip: positions are finite numbers of samples within int64'
  const onsets = new Float64Array(p.length), fracs = new Float64Array(p.length)
  p.forEach((x, k) => {
    const whole = Math.floor(x), frac = x - whole
    onsets[k] = frac >= 1 ? whole + 1 : whole
    fracs[k] = frac >= 1 ? 0 : frac
  })
  return { onsets, fracs }
}

/* channels[p]: the output channels of part p's circuit.  A placed voice is mono: refused by string otherwise (twin of render.py
 * check_space_channels). */
function checkSpaceChannels(channels, speakers) {
  channels.forEach((c, p) => {
    if (c !== 1) throw 'dusp-hip: a placed voice is mono: part ' + p + ' has ' + c + ' output channels'
  })
  return speakers
}

const SPACE_ALONE = 'dusp-hip: places stand alone: together with pans or fracs they are refused (a sub-sample onset in front of a Space would be a second two-tap stage)'
const SPACE_MAX_SPEAKERS = 8, SPACE_MAX_DELAY = 2 ** 24

/* rows of coordinates -> [Float32Array] or null where they are no list of lists of numbers */
function coordinateRows(rows) {
  if (!Array.isArray(rows) || !rows.every((r) => (Array.isArray(r) || r instanceof Float32Array || r instanceof Float64Array) && Array.from(r).every((x) => typeof x === 'number'))) return null
  return rows.map((r) => Float32Array.from(r))
}

/* places of `count` voices and the speakers -> { places, speakers }, Float32Array rows: 1 to 3 finite coordinates each, the same
 * number; speakers undefined: the reference's stereo pair (twin of mix.py check_places, with its strings). */
function checkPlaces(places, count, speakers) {
  const p = coordinateRows(places), q = coordinateRows(given(speakers) ? speakers : [[-1, 0], [1, 0]])
  if (!p || !q) throw 'dusp-hip: places and speakers are lists of 1 to 3 coordinates each'
  const dims = p.length ? p[0].length : 0
  if (p.length !== count || !(dims >= 1 && dims <= 3) || p.some((r) => r.length !== dims)) throw 'dusp-hip: places must have shape (voices=' + count + ', 1 .. 3 coordinates)'
  const qdims = q.length ? q[0].length : 0
  if (!q.length || !(qdims >= 1 && qdims <= 3) || q.some((r) => r.length !== qdims)) throw 'dusp-hip: speakers must have shape (speakers, 1 .. 3 coordinates)'
  if (q.length > SPACE_MAX_SPEAKERS) throw 'dusp-hip: a Space has 1 .. ' + SPACE_MAX_SPEAKERS + ' speakers, not ' + q.length
  if (qdims !== dims) throw 'dusp-hip: places have ' + dims + ' coordinates, speakers have ' + qdims + ': the same number'
  // (finite as numbers, before the rounding to f32: a coordinate beyond the f32 range is refused as what it becomes below)
  const rows = (v) => (given(v) ? v : [[-1, 0], [1, 0]]).map((r) => Array.from(r))
  rows(places).forEach((r, k) => { if (!r.every(Number.isFinite)) throw 'dusp-hip: the place of voice ' + k + ' is not finite' })
  rows(speakers).forEach((r, c) => { if (!r.every(Number.isFinite)) throw 'dusp-hip: the place of speaker ' + c + ' is not finite' })
  return { places: p, speakers: q }
}

/* delays and gains of `count` voices at nSpeakers speakers, Float64Arrays [voice][speaker], checked by the strings the library uses
 * (twin of mix.py check_taps) */
function checkTaps(delays, gains, count, nSpeakers) {
  if (!(delays instanceof Float64Array) || !(gains instanceof Float64Array) || delays.length !== count * nSpeakers || gains.length !== delays.length)
    throw "dusp-hip: the taps' delays and gains must both have shape (voices=" + count + ', speakers)'
  if (!(nSpeakers >= 1 && nSpeakers <= SPACE_MAX_SPEAKERS)) throw 'dusp-hip: a Space has 1 .. ' + SPACE_MAX_SPEAKERS + ' speakers, not ' + nSpeakers
  const at = (j) => 'of voice ' + Math.floor(j / nSpeakers) + ' at speaker ' + (j % nSpeakers)
  for (let j = 0; j < delays.length; j++) if (!Number.isFinite(delays[j])) throw 'dusp-hip: the delay ' + at(j) + ' is not finite'
  for (let j = 0; j < delays.length; j++) if (delays[j] < 0 || delays[j] > SPACE_MAX_DELAY) throw 'dusp-hip: the delay ' + at(j) + ' is outside [0, 2^24] samples'
  for (let j = 0; j < gains.length; j++) if (!Number.isFinite(gains[j])) throw 'dusp-hip: the gain ' + at(j) + ' is not finite'
}

/* The reference's SpaceChannel (src/patches/SpaceChannel.js) per voice and speaker, with its roundings -> { nSpeakers, delays, gains },
 * Float64Arrays [voice][speaker], what the device takes (twin of mix.py space_taps, which spells the arithmetic out).  Every coordinate
 * and factor is an inlet constant, rounded to f32; Subtract, VectorMagnitude and Multiply store f32; the gain is this engine's own
 * Math.pow(10, dB / 20), as Gain.js computes it. */
function spaceTaps(places, { speakers, decibelsPerMetre = -3, sampleDelayPerMetre, sampleRate } = {}) {
  const checked = checkPlaces(places, Array.isArray(places) ? places.length : 0, speakers)
  const f32 = Math.fround
  const sdpm = f32(given(sampleDelayPerMetre) ? sampleDelayPerMetre : (given(sampleRate) ? sampleRate : config.sampleRate) / 343), dbpm = f32(decibelsPerMetre)
  if (!Number.isFinite(sdpm) || !Number.isFinite(dbpm)) throw 'dusp-hip: decibels_per_metre and sample_delay_per_metre are finite numbers'
  const n = checked.places.length, nSpeakers = checked.speakers.length
  const delays = new Float64Array(n * nSpeakers), gains = new Float64Array(n * nSpeakers)
  for (let k = 0; k < n; k++)
    for (let c = 0; c < nSpeakers; c++) {
      let total = 0
      checked.places[k].forEach((p, i) => {
        const dx = f32(p - checked.speakers[c][i])
        total += dx * dx
      })
      const dist = f32(Math.sqrt(total)), dB = f32(dist * dbpm)
      delays[k * nSpeakers + c] = f32(dist * sdpm)
      gains[k * nSpeakers + c] = Number.isFinite(dB) ? Math.pow(10, dB / 20) : NaN
    }
  checkTaps(delays, gains, n, nSpeakers)
  return { nSpeakers, delays, gains }
}

/* The refusals of a master, in the words of mix.py (MASTER_*) */
const MASTER = {
  inputAlone: MasterInput.ALONE,
  notCallable: 'dusp-hip: master is a function fx(x) of the mix, or a list of one function a channel of the timeline',
  count: (have, channels) => 'dusp-hip: master lists ' + have + ' circuits, the timeline has ' + channels + ' channels: one a channel',
  oneInput: (c, have) => 'dusp-hip: the master of channel ' + c + ' holds ' + have + ' MasterInput units: a master reads the mix through exactly one, the one it is given',
  hostSource: (c) => 'dusp-hip: the master of channel ' + c + " holds a HostSource: the timeline is a master's only input",
  events: (c) => 'dusp-hip: the master of channel ' + c + ' has scheduled events: a master is rendered in one piece',
  channels: (c, have) => 'dusp-hip: the master of channel ' + c + ' has ' + have + ' output channels: a master is a mono circuit, applied to every channel by itself',
  notIsomorphic: (c) => 'dusp-hip: the masters of channels 0 and ' + c + ' are not isomorphic circuits: they are one program and may differ in constants only',
  rate: (have, want) => "dusp-hip: the master's sample rate is " + have + ", the voices' is " + want,
}

/* The master of a score or piece -> unify's result over `channels` instances, one a channel of the timeline (twin of render.py
 * master_program).  master: a function fx(x), called once per channel with a fresh MasterInput and returning the master's outlet, or an
 * array of one function a channel.  The circuits are isomorphic; what differs between them is constants, which become the program's
 * parameter table [nParams][channels].  Refused by string: what is no function, an array of the wrong length, a circuit that holds no
 * or several MasterInput, another host-computed signal or a scheduled event, one with more than one output channel, circuits that are
 * not isomorphic. */
function masterProgram(master, channels, sampleRate, bus = null) {
  return unify(channelCircuits(master, channels, sampleRate, bus))
}

/* masterProgram's circuits, extracted and checked, one a channel, before they are unified (twin of render.py _channel_circuits) */
function channelCircuits(master, channels, sampleRate, bus = null, track = null) {
  // bus (null: a master): the circuit is bus number `bus` of the call's buses — given and checked as a master is, refused in BUS's words;
  // track: the circuit is track number `track` of the call's tracks, refused in TRACK's words
  const words = track !== null ? TRACK : bus !== null ? BUS : MASTER, named = track !== null ? [track] : bus !== null ? [bus] : []
  const refuse = (name, ...args) => words[name].apply(null, named.concat(args))
  const fxs = Array.isArray(master) ? master : new Array(channels).fill(master)
  if (!fxs.length || !fxs.every((fx) => typeof fx === 'function')) throw (named.length ? words.notCallable(named[0]) : MASTER.notCallable)
  if (fxs.length !== channels) throw refuse('count', fxs.length, channels)
  const extractions = []
  fxs.forEach((fx, c) => {
    const ex = extract(fx(new MasterInput()), { allowEvents: true })
    if (ex.circuit.events && ex.circuit.events.length) throw refuse('events', c)
    if (ex.sources.some((u) => !u.isMasterInput)) throw refuse('hostSource', c)
    if (ex.sources.length !== 1) throw refuse('oneInput', c, ex.sources.length)
    if (ex.sampleRate !== sampleRate) throw refuse('rate', ex.sampleRate, sampleRate)
    const nOut = native().descriptorChannels(ex.words)
    if (nOut !== 1) throw refuse('channels', c, nOut)
    if (c && structureKey(ex) !== structureKey(extractions[0])) throw refuse('notIsomorphic', c)
    extractions.push(ex)
  })
  return extractions
}

/* Effect sends (DESIGN.md 6.15): the refusals of a bus and of the levels, in the words of mix.py (BUS_*, SENDS_*) */
const BUS = {
  notCallable: (b) => 'dusp-hip: bus ' + b + ' is a function fx(x) of its send timeline, or a list of one function a channel of the timeline',
  count: (b, have, channels) => 'dusp-hip: bus ' + b + ' lists ' + have + ' circuits, the timeline has ' + channels + ' channels: one a channel',
  oneInput: (b, c, have) => 'dusp-hip: bus ' + b + ', channel ' + c + ', holds ' + have + ' MasterInput units: a bus reads its sends through exactly one, the one it is given',
  hostSource: (b, c) => 'dusp-hip: bus ' + b + ', channel ' + c + ", holds a HostSource: the send timeline is a bus's only input",
  events: (b, c) => 'dusp-hip: bus ' + b + ', channel ' + c + ', has scheduled events: a bus is rendered in one piece',
  channels: (b, c, have) => 'dusp-hip: bus ' + b + ', channel ' + c + ', has ' + have + ' output channels: a bus is a mono circuit, applied to every channel by itself',
  notIsomorphic: (b, c) => 'dusp-hip: the circuits of bus ' + b + ' at channels 0 and ' + c + ' are not isomorphic: they are one program and may differ in constants only',
  rate: (b, have, want) => 'dusp-hip: the sample rate of bus ' + b + ' is ' + have + ", the voices' is " + want,
}
const SENDS = {
  withoutBuses: 'dusp-hip: sends without buses: a send level is what a voice gives to a bus',
  withoutSends: 'dusp-hip: buses without sends: every bus needs a send level a voice (sends of shape (buses, voices))',
  busCount: (have) => 'dusp-hip: a call has 1 .. 4 buses, not ' + have,
  placement: 'dusp-hip: sends go with plain rows and with pans at whole-sample onsets: together with fracs, places or stereo they are refused',
  shape: (buses, voices) => 'dusp-hip: sends must have shape (buses=' + buses + ', voices=' + voices + ')',
  notFinite: (k, b) => 'dusp-hip: the send level of voice ' + k + ' into bus ' + b + ' is not finite',
}

/* the send levels of `count` voices into nBuses buses -> Float32Array [nBuses * count], bus by bus (twin of mix.py check_sends): an
 * array of nBuses arrays of `count` numbers, or — one bus — `count` numbers; every level finite as a float32 */
function checkSends(sends, count, nBuses) {
  if (!(nBuses >= 1 && nBuses <= 4)) throw SENDS.busCount(nBuses)
  const isList = (x) => Array.isArray(x) || ArrayBuffer.isView(x)
  if (!isList(sends)) throw SENDS.shape(nBuses, count)
  let rows = Array.from(sends)
  if (nBuses === 1 && rows.length === count && !rows.some(isList) && !(count === 1 && isList(sends[0]))) rows = [rows]
  if (rows.length !== nBuses || !rows.every((r) => isList(r) && r.length === count && !Array.from(r).some(isList))) throw SENDS.shape(nBuses, count)
  const out = new Float32Array(nBuses * count)
  rows.forEach((r, b) => out.set(Float32Array.from(r, Number), b * count))
  for (let b = 0; b < nBuses; b++) for (let k = 0; k < count; k++) if (!Number.isFinite(out[b * count + k])) throw SENDS.notFinite(k, b)
  return out
}

/* Tracks (DESIGN.md 6.16): the refusals of a track's circuit and of what says where the voices go, in the words of mix.py (TRACK_*, TRACKS_*) */
const TRACK = {
  notCallable: (g) => 'dusp-hip: track ' + g + ' is None (a fader group), a function fx(x) of its sub-mix, or a list of one function a channel of the timeline',
  count: (g, have, channels) => 'dusp-hip: track ' + g + ' lists ' + have + ' circuits, the timeline has ' + channels + ' channels: one a channel',
  oneInput: (g, c, have) => 'dusp-hip: track ' + g + ', channel ' + c + ', holds ' + have + ' MasterInput units: a track reads its sub-mix through exactly one, the one it is given',
  hostSource: (g, c) => 'dusp-hip: track ' + g + ', channel ' + c + ", holds a HostSource: the track's timeline is its circuit's only input",
  events: (g, c) => 'dusp-hip: track ' + g + ', channel ' + c + ', has scheduled events: a track is rendered in one piece',
  channels: (g, c, have) => 'dusp-hip: track ' + g + ', channel ' + c + ', has ' + have + " output channels: a track's circuit is mono, applied to every channel by itself",
  notIsomorphic: (g, c) => 'dusp-hip: the circuits of track ' + g + ' at channels 0 and ' + c + ' are not isomorphic: they are one program and may differ in constants only',
  rate: (g, have, want) => 'dusp-hip: the sample rate of track ' + g + ' is ' + have + ", the voices' is " + want,
}
const TRACKS = {
  withoutTrackOf: 'dusp-hip: tracks without track_of: every voice goes to a track or, with -1, straight to the mix',
  trackOfAlone: 'dusp-hip: track_of without tracks: a track is what a voice goes to',
  needTracks: (name) => 'dusp-hip: ' + name + ' without tracks: it says something about every track',
  count: (have) => 'dusp-hip: a call has 1 .. 8 tracks, not ' + have,
  trackOfShape: (voices) => 'dusp-hip: track_of must have shape (voices=' + voices + ',) and hold whole numbers',
  trackOfRange: (k, g, tracks) => 'dusp-hip: voice ' + k + ' names track ' + g + ' of ' + tracks + ': track_of holds -1 (straight to the mix) or a track, 0 .. ' + (tracks - 1),
  fadersShape: (tracks) => 'dusp-hip: faders must have shape (tracks=' + tracks + ',)',
  faderNotFinite: (g) => 'dusp-hip: the fader of track ' + g + ' is not finite',
  sendsShape: (buses, tracks) => 'dusp-hip: track_sends must have shape (buses=' + buses + ', tracks=' + tracks + ')',
  levelNotFinite: (g, b) => 'dusp-hip: the level of track ' + g + ' into bus ' + b + ' is not finite',
  sendsWithoutBuses: 'dusp-hip: track_sends without buses: a level is what a track gives to a bus',
  busesWithoutSends: 'dusp-hip: buses without track_sends: with tracks every bus needs a level a track (track_sends of shape (buses, tracks))',
  withSends: 'dusp-hip: sends and tracks do not go together: with tracks the buses are fed by track_sends, a level a track',
}

/* What says where the `count` voices of a call with nTracks tracks go, and what the tracks give -> { trackOf Int32Array [count], faders
 * Float32Array [nTracks] | null, trackSends Float32Array [nBuses * nTracks] | null } (twin of mix.py check_tracks: the same checks in
 * the same order, the same strings).  nTracks null: the call has no tracks, and every other option of theirs is refused. */
function checkTracks(count, nTracks, trackOf, faders = null, trackSends = null, nBuses = 0, sends = null) {
  const isList = (x) => Array.isArray(x) || ArrayBuffer.isView(x)
  if (!given(nTracks)) {
    if (given(trackOf)) throw TRACKS.trackOfAlone
    if (given(faders)) throw TRACKS.needTracks('faders')
    if (given(trackSends)) throw TRACKS.needTracks('track_sends')
    return { trackOf: null, faders: null, trackSends: null }
  }
  if (!given(trackOf)) throw TRACKS.withoutTrackOf
  if (!(nTracks >= 1 && nTracks <= 8)) throw TRACKS.count(nTracks)
  if (!isList(trackOf) || trackOf.length !== count || Array.from(trackOf).some((x) => typeof x !== 'number' || !Number.isInteger(x))) throw TRACKS.trackOfShape(count)
  const of = Array.from(trackOf)
  for (let k = 0; k < count; k++) if (of[k] < -1 || of[k] >= nTracks) throw TRACKS.trackOfRange(k, of[k], nTracks)
  let f = null, levels = null
  if (given(faders)) {
    if (!isList(faders) || faders.length !== nTracks || Array.from(faders).some(isList)) throw TRACKS.fadersShape(nTracks)
    f = Float32Array.from(faders, Number)
    for (let g = 0; g < nTracks; g++) if (!Number.isFinite(f[g])) throw TRACKS.faderNotFinite(g)
  }
  if (given(sends)) throw TRACKS.withSends
  if (given(trackSends) && !nBuses) throw TRACKS.sendsWithoutBuses
  if (nBuses && !given(trackSends)) throw TRACKS.busesWithoutSends
  if (given(trackSends)) {
    if (!(nBuses >= 1 && nBuses <= 4)) throw SENDS.busCount(nBuses)
    if (!isList(trackSends)) throw TRACKS.sendsShape(nBuses, nTracks)
    let rows = Array.from(trackSends)
    if (nBuses === 1 && !rows.some(isList)) rows = [rows]
    if (rows.length !== nBuses || !rows.every((r) => isList(r) && r.length === nTracks && !Array.from(r).some(isList))) throw TRACKS.sendsShape(nBuses, nTracks)
    levels = new Float32Array(nBuses * nTracks)
    rows.forEach((r, b) => levels.set(Float32Array.from(r, Number), b * nTracks))
    for (let b = 0; b < nBuses; b++) for (let g = 0; g < nTracks; g++) if (!Number.isFinite(levels[b * nTracks + g])) throw TRACKS.levelNotFinite(g, b)
  }
  return { trackOf: Int32Array.from(of), faders: f, trackSends: levels }
}

/* The tracks of a score or piece -> [{ uni, tracks }]: the tracks' circuits grouped by structure in the order their first track comes,
 * every group ONE program whose instances are (track, channel), instance j * channels + c the circuit of the group's j-th track over
 * channel c (twin of render.py track_programs).  tracks: an array of 1 .. 8 entries, each null (a track without a circuit) or given as
 * a master is. */
function trackPrograms(tracks, channels, sampleRate) {
  const index = new Map(), members = []
  tracks.forEach((fx, g) => {
    if (!given(fx)) return
    const extractions = channelCircuits(fx, channels, sampleRate, null, g)
    const key = structureKey(extractions[0])
    if (!index.has(key)) {
      index.set(key, members.length)
      members.push({ extractions: [], tracks: [] })
    }
    const m = members[index.get(key)]
    m.extractions.push(...extractions)
    m.tracks.push(g)
  })
  return members.map((m) => ({ uni: unify(m.extractions), tracks: m.tracks }))
}

/* Stems (DESIGN.md 6.17): the refusal and the names, in the words of mix.py (STEMS_NOT_BOOL, stem_names) */
const STEMS_NOT_BOOL = 'dusp-hip: stems is True or False: with True a call delivers the direct mix, every track and every bus return beside the mix'
function checkStems(stems) {
  if (stems === undefined) return false
  if (typeof stems !== 'boolean') throw STEMS_NOT_BOOL
  return stems
}
function stemNames(nTracks, nBuses) {
  const names = ['direct']
  for (let g = 0; g < nTracks; g++) names.push('track' + g)
  for (let b = 0; b < nBuses; b++) names.push('bus' + b)
  return names.concat(['mix'])
}
/* the one peak of several signals: the largest of their peaks compared as unsigned bit patterns, a NaN wins (twin of wav.py common_peak) */
function commonPeak(peaks) {
  const f = Float32Array.from(peaks), bits = new Uint32Array(f.buffer)
  let top = 0
  for (const b of bits) if (b > top) top = b
  return new Float32Array(new Uint32Array([top]).buffer)[0]
}
/* What a call with stems: true resolves to (twin of render.py Stems): names, the signals in the order they were delivered; mix, exactly
 * what the call resolves to without stems; direct, tracks (one a track) and buses (one a bus), each of the mix's kind; peaks, name ->
 * the signal's own peak; peak, the largest of them; for PCM gain, the one gain all frames were encoded under. */
function stemsOf(names, signals, peaks, extra = {}) {
  const nTracks = names.filter((name) => name.startsWith('track')).length
  const out = { names, direct: signals[0], tracks: signals.slice(1, 1 + nTracks), buses: signals.slice(1 + nTracks, -1), mix: signals[signals.length - 1], peaks: {}, peak: commonPeak(peaks) }
  names.forEach((name, s) => { out.peaks[name] = peaks[s] })
  return Object.assign(out, extra)
}
function planarStems(names, nSamples, nChannels, sampleRate, result) {
  const signals = names.map((name, s) => {
    const channelData = []
    channelData.sampleRate = sampleRate
    if (result) for (let c = 0; c < nChannels; c++) channelData.push(result.data.subarray((s * nChannels + c) * nSamples, (s * nChannels + c + 1) * nSamples))
    return channelData
  })
  return stemsOf(names, signals, result ? result.peaks : new Float32Array(names.length))
}
function pcmStems(names, nChannels, sampleRate, result, bitDepth, normalise) {
  const peaks = result ? result.peaks : new Float32Array(names.length), each = result ? result.data.length / names.length : 0
  const signals = names.map((name, s) => ({ data: result ? result.data.subarray(s * each, (s + 1) * each) : Buffer.alloc(0), bitDepth, numberOfChannels: result ? nChannels : 0, sampleRate, peak: peaks[s] }))
  const peak = commonPeak(peaks)
  return stemsOf(names, signals, peaks, { gain: normalise && Number.isFinite(peak) && peak > (normalise === 1 ? 1 : 0) ? 1 / peak : 1 })
}
/* PCM -> a WAV file; the stems of a call -> a file a signal */
function wavOf(pcm) {
  if (pcm.meters && !pcm.names) return Object.assign({ mix: encodeWav(pcm.mix), meters: pcm.meters }, pcm.level === undefined ? {} : { gain: pcm.gain, level: pcm.level }, pcm.limiter === undefined ? {} : { limiter: pcm.limiter }) // (meters without stems)
  if (pcm.meters) return Object.assign(wavOf(Object.assign({}, pcm, { meters: undefined })), { meters: pcm.meters })
  if (!pcm.names) return encodeWav(pcm)
  const files = pcm.names.map((name, s) => encodeWav(s === 0 ? pcm.direct : s === pcm.names.length - 1 ? pcm.mix : s <= pcm.tracks.length ? pcm.tracks[s - 1] : pcm.buses[s - 1 - pcm.tracks.length]))
  return stemsOf(pcm.names, files, pcm.names.map((name) => pcm.peaks[name]), Object.assign({ gain: pcm.gain }, pcm.level === undefined ? {} : { level: pcm.level }, pcm.limiter === undefined ? {} : { limiter: pcm.limiter }))
}

/* Meters (DESIGN.md 6.18): the refusals, the hop and the block count, in the words of mix.py (METERS_NOT_BOOL, METER_RATE_LOW, meter_hop,
 * meter_blocks) */
const METERS_NOT_BOOL = 'dusp-hip: meters is True or False: with True a call also delivers the RMS and the BS.1770 loudness of every signal it delivers'
const METER_RATE_LOW = (rate) => 'dusp-hip: meters need a sample rate of at least 8000 Hz, not ' + rate + ": the K-weighting's shelf lies at 1682 Hz"
function checkMeters(meters) {
  if (meters === undefined) return false
  if (typeof meters !== 'boolean') throw METERS_NOT_BOOL
  return meters
}
/* Loudness delivery (DESIGN.md 6.19): the refusals in the words of mix.py (TRUE_PEAK_NOT_BOOL, LOUDNESS_NOT_NUMBER, TRUE_PEAK_MAX_BAD,
 * LOUDNESS_WITH_NORMALISE, LOUDNESS_PLANAR; check_true_peak, check_loudness) */
const TRUE_PEAK_NOT_BOOL = 'dusp-hip: true_peak is True or False: with True a call also delivers the true peak of every signal and channel it delivers'
const LOUDNESS = {
  notNumber: 'dusp-hip: loudness is None or a finite number, the target in LUFS (-14, -16, -23 ...): the frames are then encoded at that loudness',
  ceiling: 'dusp-hip: true_peak_max is a finite number of dBTP at most 0 (default -1), the ceiling no delivered signal\'s true peak exceeds',
  withNormalise: (normalise) => 'dusp-hip: loudness and normalise=' + normalise + ' do not go together: the target decides the gain, normalise must be 0',
  planar: 'dusp-hip: loudness goes with the _pcm and _wav calls: 32-bit frames via bit_depth=32 are the f32 delivery at a target'
}
/* The limiter of a loudness delivery (DESIGN.md 6.20): the refusals in the words of mix.py (LIMITER_NOT_BOOL, LIMITER_NEEDS_LOUDNESS,
 * LIMITER_WINDOW_BAD, LIMITER_WINDOW_LONG; check_limiter) */
const LIMITER = {
  notBool: 'dusp-hip: limiter is True or False: with True a delivery at a loudness target is limited to the true-peak ceiling before the one gain is taken',
  needsLoudness: "dusp-hip: limiter without loudness: the limiter's threshold is the ceiling seen from the loudness target, so it needs loudness=",
  windowBad: "dusp-hip: limiter_window is a finite positive number of seconds (default 0.005), the limiter's look-ahead, attack and release",
  windowLong: (samples, sampleRate) => 'dusp-hip: limiter_window is ' + samples + ' samples at ' + sampleRate + " Hz: the limiter's window is at most 4096 samples",
  threshold: "dusp-hip: the limiter's threshold is a finite number above 0, linear",
  windowSamples: "dusp-hip: the limiter's window is a whole number of samples, 1 .. 4096",
  // (DESIGN.md 6.21: LIMITER_RELEASE_BAD, LIMITER_RELEASE_NEEDS_LIMITER, LIMITER_RELEASE_LONG, LIMITER_RELEASE_SAMPLES; check_limiter_release)
  releaseBad: "dusp-hip: limiter_release is None or a finite positive number of seconds, the time the limiter's gain takes from 0 back to 1",
  releaseNeedsLimiter: "dusp-hip: limiter_release without limiter=True: a release is the limiter's",
  releaseLong: (samples, sampleRate) => 'dusp-hip: limiter_release is ' + samples + ' samples at ' + sampleRate + " Hz: the limiter's release is at most 4194304 samples",
  releaseSamples: "dusp-hip: the limiter's release is a whole number of samples, 1 .. 4194304"
}
function checkLimiterBool(limiter) {
  if (limiter === undefined) return false
  if (typeof limiter !== 'boolean') throw LIMITER.notBool
  return limiter
}
/* limiter (a boolean already), limiterWindow: of a call with that loudness target at that sample rate -> the window in samples, 0 without a
 * limiter: max(1, round(window x sampleRate)), halves to the even number as Python's round */
function checkLimiter(limiter, limiterWindow, target, sampleRate) {
  if (!limiter) return 0
  if (target === null) throw LIMITER.needsLoudness
  const w = limiterWindow === undefined ? 0.005 : limiterWindow
  if (typeof w !== 'number' || !Number.isFinite(w) || !(w > 0)) throw LIMITER.windowBad
  const exact = w * sampleRate
  if (exact > 2 * 4096) throw LIMITER.windowLong(BigInt(Math.min(Math.trunc(exact), 2 ** 62)).toString(), sampleRate) // (Python's min(int(.), 2**62) through %d)
  const down = Math.floor(exact), rounded = exact - down > 0.5 || (exact - down === 0.5 && down % 2 === 1) ? down + 1 : down
  const L = Math.max(1, rounded)
  if (L > 4096) throw LIMITER.windowLong(L, sampleRate)
  return L
}
/* limiterRelease: of a call with that limiter (a boolean already) at that sample rate -> the release in samples, 0 without one:
 * max(1, round(seconds x sampleRate)), halves to the even number as Python's round (twin of mix.py check_limiter_release) */
function checkLimiterRelease(limiterRelease, limiter, sampleRate) {
  if (!given(limiterRelease)) return 0
  const r = limiterRelease
  if (typeof r !== 'number' || !Number.isFinite(r) || !(r > 0)) throw LIMITER.releaseBad
  if (!limiter) throw LIMITER.releaseNeedsLimiter
  const exact = r * sampleRate
  if (exact > 2 * 4194304) throw LIMITER.releaseLong(BigInt(Math.min(Math.trunc(exact), 2 ** 62)).toString(), sampleRate)
  const down = Math.floor(exact), rounded = exact - down > 0.5 || (exact - down === 0.5 && down % 2 === 1) ? down + 1 : down
  const R = Math.max(1, rounded)
  if (R > 4194304) throw LIMITER.releaseLong(R, sampleRate)
  return R
}
function checkTruePeak(truePeak) {
  if (truePeak === undefined) return false
  if (typeof truePeak !== 'boolean') throw TRUE_PEAK_NOT_BOOL
  return truePeak
}
/* loudness:, truePeakMax: of a call -> { target (null: none), ceiling }; pcm: whether the call delivers frames */
function checkLoudness(loudness, truePeakMax, normalise, pcm) {
  const ceiling = truePeakMax === undefined ? -1 : truePeakMax
  if (typeof ceiling !== 'number' || !Number.isFinite(ceiling) || ceiling > 0) throw LOUDNESS.ceiling
  if (!given(loudness)) return { target: null, ceiling }
  if (typeof loudness !== 'number' || !Number.isFinite(loudness)) throw LOUDNESS.notNumber
  if (!pcm) throw LOUDNESS.planar
  if (normalise !== 0) throw LOUDNESS.withNormalise(normalise)
  return { target: loudness, ceiling }
}
const meterHop = (sampleRate) => Math.floor((sampleRate + 5) / 10)
function meterBlocks(n, sampleRate) {
  const hop = meterHop(sampleRate), block = 4 * hop
  return n < block ? 0 : Math.floor((n - block) / hop) + 1
}
/* What a call with meters: true holds as `meters` (twin of render.py Meters): names, the signals in the order they were delivered
 * (stemNames with stems, else ['mix']); rms, name -> Float64Array [channels]; lufs, name -> the gated integrated loudness of ITU-R
 * BS.1770-4 (-Infinity: no block above the gates, NaN: a sample that is not finite); momentary, name -> Float64Array [blocks], the
 * loudness of every 400 ms block, 100 ms apart; hop and block in samples.  Taken on the f32 signals in front of the PCM gain: the
 * loudness of an encoded file is lufs + 20 log10(gain).  got (the addon's doubles; null: a timeline of no samples, no energy, no block).
 * truePeak (a call with truePeak: true or loudness:): also truePeak, name -> Float64Array [channels], linear: dBTP is 20 log10. */
function metersOf(names, got, nChannels, nBlocks, sampleRate, truePeak = false) {
  const out = { names, rms: {}, lufs: {}, momentary: {}, hop: meterHop(sampleRate), block: 4 * meterHop(sampleRate) }
  if (truePeak) out.truePeak = {}
  names.forEach((name, s) => {
    if (truePeak) out.truePeak[name] = got ? got.truePeak.slice(s * nChannels, (s + 1) * nChannels) : new Float64Array(nChannels)
    out.rms[name] = got ? got.rms.slice(s * nChannels, (s + 1) * nChannels) : new Float64Array(nChannels)
    out.lufs[name] = got ? got.lufs[s] : -Infinity
    out.momentary[name] = got ? got.momentary.slice(s * nBlocks, (s + 1) * nBlocks) : new Float64Array(0)
  })
  return out
}
/* what a call resolves to, with its meters where it has some: the stems gain `.meters`; without stems { mix, meters } (twin of render.py Metered) */
function withMeters(delivered, metered, loud = null) {
  if (!metered) return delivered
  const out = delivered && delivered.names ? Object.assign(delivered, { meters: metered }) : { mix: delivered, meters: metered }
  return loud ? Object.assign(out, loud) : out // (a call with loudness: the one gain the frames were encoded under, and the level it came from)
}
/* The meters of any signals a user has (twin of render.py meter): channelData — an array of Float32Arrays, the channels of one signal, or
 * an array of such arrays, several signals of the same shape — at sampleRate -> what metersOf makes, the names '0', '1', ...; metered on
 * the device and gated in the library (dusp_meter_host). */
function meter(channelData, sampleRate) {
  const signals = channelData.length && !ArrayBuffer.isView(channelData[0]) ? Array.from(channelData) : [channelData]
  const nChannels = signals[0].length, nSamples = nChannels ? signals[0][0].length : 0
  if (!(sampleRate >= 8000)) throw METER_RATE_LOW(sampleRate)
  if (!nChannels || signals.some((sig) => sig.length !== nChannels || Array.from(sig).some((ch) => !(ch instanceof Float32Array) || ch.length !== nSamples)))
    throw 'dusp-hip: meter: the signals to meter are Float32Arrays of one length, the same number a signal'
  const names = signals.map((sig, s) => String(s))
  if (nSamples === 0) return metersOf(names, null, nChannels, 0, sampleRate)
  const planar = new Float32Array(signals.length * nChannels * nSamples)
  signals.forEach((sig, s) => Array.from(sig).forEach((ch, c) => planar.set(ch, (s * nChannels + c) * nSamples)))
  const got = native().meter(contextFor(sampleRate), planar, signals.length, nChannels, nSamples, sampleRate)
  return metersOf(names, got, nChannels, meterBlocks(nSamples, sampleRate), sampleRate)
}
/* The true peak of any signals a user has (twin of render.py true_peak): channelData as meter takes it -> an array, one Float64Array
 * [channels] a signal, linear; taken on the device (dusp_true_peak_host). */
function truePeak(channelData, sampleRate) {
  const signals = channelData.length && !ArrayBuffer.isView(channelData[0]) ? Array.from(channelData) : [channelData]
  const nChannels = signals[0].length, nSamples = nChannels ? signals[0][0].length : 0
  if (!(sampleRate > 0)) throw 'dusp-hip: truePeak: the true peak needs a sample rate: it decides the oversampling'
  if (!nChannels || signals.some((sig) => sig.length !== nChannels || Array.from(sig).some((ch) => !(ch instanceof Float32Array) || ch.length !== nSamples)))
    throw 'dusp-hip: truePeak: the signals are Float32Arrays of one length, the same number a signal'
  if (nSamples === 0) return signals.map(() => new Float64Array(nChannels))
  const planar = new Float32Array(signals.length * nChannels * nSamples)
  signals.forEach((sig, s) => Array.from(sig).forEach((ch, c) => planar.set(ch, (s * nChannels + c) * nSamples)))
  const got = native().truePeak(contextFor(sampleRate), planar, signals.length, nChannels, nSamples, sampleRate)
  return signals.map((sig, s) => got.slice(s * nChannels, (s + 1) * nChannels))
}

/* The linked look-ahead limiter over any signals a user has (twin of render.py limit): channelData as meter takes it, a threshold (linear,
 * finite, above 0) and a window of 1 .. 4096 samples -> { data, gain, reduction }: data shaped as channelData, every row multiplied by ONE
 * gain curve; gain the curve, a Float64Array [samples]; reduction its smallest value, 1 where nothing exceeds the threshold.  On the
 * device (dusp_limit_host).  release: undefined, or the limiter's release of its own, 1 .. 2^22 samples (dusp_limit_release_host;
 * DESIGN.md 6.21). */
function limit(channelData, sampleRate, threshold, window, release) {
  const nested = channelData.length && !ArrayBuffer.isView(channelData[0])
  const signals = nested ? Array.from(channelData) : [channelData]
  const nChannels = signals[0].length, nSamples = nChannels ? signals[0][0].length : 0
  if (!(sampleRate > 0)) throw 'dusp-hip: limit: the limiter needs a sample rate: it decides the oversampling'
  if (typeof threshold !== 'number' || !Number.isFinite(threshold) || !(threshold > 0)) throw LIMITER.threshold
  if (!Number.isInteger(window) || window < 1 || window > 4096) throw LIMITER.windowSamples
  if (given(release) && (!Number.isInteger(release) || release < 1 || release > 4194304)) throw LIMITER.releaseSamples
  if (!nChannels || signals.some((sig) => sig.length !== nChannels || Array.from(sig).some((ch) => !(ch instanceof Float32Array) || ch.length !== nSamples)))
    throw 'dusp-hip: limit: the signals are Float32Arrays of one length, the same number a signal'
  if (nSamples === 0) return { data: nested ? signals.map((sig) => Array.from(sig, () => new Float32Array(0))) : Array.from(signals[0], () => new Float32Array(0)), gain: new Float64Array(0), reduction: 1 }
  const planar = new Float32Array(signals.length * nChannels * nSamples)
  signals.forEach((sig, s) => Array.from(sig).forEach((ch, c) => planar.set(ch, (s * nChannels + c) * nSamples)))
  const got = given(release) ? native().limitRelease(contextFor(sampleRate), planar, signals.length, nChannels, nSamples, sampleRate, threshold, window, release)
    : native().limit(contextFor(sampleRate), planar, signals.length, nChannels, nSamples, sampleRate, threshold, window)
  const rows = signals.map((sig, s) => Array.from(sig, (ch, c) => got.data.subarray((s * nChannels + c) * nSamples, (s * nChannels + c + 1) * nSamples)))
  return { data: nested ? rows : rows[0], gain: got.gain, reduction: got.reduction }
}

/* what sends and tracks do not go with, refused before anything else of a call is looked at (twin of render.py _placing) */
function refuseSends(opts) {
  if (!given(opts.tracks)) {
    checkTracks(0, null, opts.trackOf, opts.faders, opts.trackSends)
    if (!given(opts.buses) && given(opts.sends)) throw SENDS.withoutBuses
  } else {
    if (!Array.isArray(opts.tracks) || opts.tracks.length < 1 || opts.tracks.length > 8) throw TRACKS.count(Array.isArray(opts.tracks) ? opts.tracks.length : 0)
    if (!given(opts.trackOf)) throw TRACKS.withoutTrackOf
    if (given(opts.sends)) throw TRACKS.withSends
    if (given(opts.trackSends) && !given(opts.buses)) throw TRACKS.sendsWithoutBuses
    if (given(opts.buses) && !given(opts.trackSends)) throw TRACKS.busesWithoutSends
  }
  if (!given(opts.buses)) return
  if (!given(opts.tracks)) {
    if (!given(opts.sends)) throw SENDS.withoutSends
    if (given(opts.fracs) || given(opts.places) || opts.stereo === true) throw SENDS.placement
  }
  if (!Array.isArray(opts.buses) || opts.buses.length < 1 || opts.buses.length > 4) throw SENDS.busCount(Array.isArray(opts.buses) ? opts.buses.length : 0)
}

async function pieceCall(who, outlets, opts, format, normalise, onePart = false) {
  const { gains, engine = 0, tileBytes = 0, duration = 1, voiceDurations = 1 } = opts
  const stereo = opts.stereo === true
  const stems = checkStems(opts.stems) // (what is no boolean is refused first)
  const metersAsked = checkMeters(opts.meters) // (... and next to it)
  const truePeakAsked = checkTruePeak(opts.truePeak) // (... and next to that)
  const limiterAsked = checkLimiterBool(opts.limiter) // (... and next to that again)
  const loud = checkLoudness(opts.loudness, opts.truePeakMax, normalise, format !== 0) // (... then what the loudness target does not go with)
  const truePeaks = truePeakAsked || loud.target !== null, meters = metersAsked || truePeaks // (a target implies true peaks, true peaks imply meters)
  refuseSends(opts)
  if (given(opts.places) && stereo) throw STEREO_NO_PLACES
  if (given(opts.places) && (given(opts.pans) || given(opts.fracs))) throw SPACE_ALONE
  const extractions = outlets.map((o) => extract(o))
  if (extractions.length === 0) throw 'dusp-hip: no instances'
  for (const ex of extractions)
    for (const u of ex.circuit.units)
      if ((u.isHostSignal || (UNITS[u.constructor.name] && UNITS[u.constructor.name].hostTick)) && !deviceRetrigger(u, ex.circuit.units))
        throw 'dusp-hip: ' + who + ' does not take circuits with host-ticked units (' + u.label + '): render them one by one'
  const count = extractions.length, sampleRate = extractions[0].sampleRate
  const durations = typeof voiceDurations === 'number' ? new Array(count).fill(voiceDurations) : Array.from(voiceDurations)
  if (durations.length !== count) throw 'dusp-hip: ' + who + ': voiceDurations must be one number or hold one value per outlet'
  const voiceSamples = durations.map((x) => sampleCount(x, sampleRate))
  if (voiceSamples.some((x) => x === 0)) throw 'dusp-hip: ' + who + ': voiceDuration must cover at least one sample'
  const nSamples = sampleCount(duration, sampleRate)
  const onsets = wholeSamples(who, 'onsets', opts.onsets, count)
  let lengths = null
  if (opts.lengths !== undefined && opts.lengths !== null) {
    lengths = wholeSamples(who, 'lengths', opts.lengths, count)
    for (let k = 0; k < count; k++) if (Number(lengths[k]) < 0 || Number(lengths[k]) > voiceSamples[k]) throw 'dusp-hip: ' + who + ": lengths must lie in 0 .. the voice's own samples"
  }
  let g = null
  if (gains !== undefined && gains !== null) {
    g = gains instanceof Float32Array ? gains : Float32Array.from(gains)
    if (g.length !== count) throw 'dusp-hip: ' + who + ': gains must hold one value per outlet'
  }
  if (!Number.isInteger(tileBytes) || tileBytes < 0) throw 'dusp-hip: ' + who + ': tileBytes must be 0 (the default tile) or a whole number of bytes'
  const panned = stereo ? stereoPanArrays(opts.pans, count) : opts.pans !== undefined && opts.pans !== null ? panArrays(opts.pans, count) : null
  const fracs = opts.fracs !== undefined && opts.fracs !== null ? fracArrays(opts.fracs, count) : null
  let taps = null
  if (given(opts.places)) {
    checkPlaces(opts.places, count, opts.speakers)
    taps = spaceTaps(opts.places, { speakers: opts.speakers, decibelsPerMetre: opts.decibelsPerMetre, sampleDelayPerMetre: opts.sampleDelayPerMetre, sampleRate })
  }
  const grouped = pieceParts(extractions, voiceSamples)
  if (onePart && grouped.parts.length !== 1) throw 'dusp-hip: the voices of a score are isomorphic circuits: a piece renders several instruments'
  const n = native()
  const channels = grouped.parts.map((part) => n.descriptorChannels(part.uni.words))
  const nChannels = stereo ? checkStereoKinds(Array.from(grouped.partOf, (p) => channels[p]), panned.pans) : taps ? checkSpaceChannels(channels, taps.nSpeakers) : panned ? checkPanChannels(channels) : checkPieceChannels(channels)
  const master = given(opts.master) ? masterProgram(opts.master, nChannels, sampleRate) : null // (behind every other check of the call)
  let routed = null, groups = null // (... the tracks: the arrays, then the track circuits grouped into programs)
  if (given(opts.tracks)) {
    routed = checkTracks(count, opts.tracks.length, opts.trackOf, opts.faders, opts.trackSends, given(opts.buses) ? opts.buses.length : 0, opts.sends)
    groups = trackPrograms(opts.tracks, nChannels, sampleRate)
  }
  let buses = null, sends = null // (... the buses behind the master: the levels, then each bus as a master is made)
  if (given(opts.buses)) {
    sends = routed ? null : checkSends(opts.sends, count, opts.buses.length)
    buses = opts.buses.map((fx, b) => masterProgram(fx, nChannels, sampleRate, b))
  }
  const names = stems ? stemNames(routed ? opts.tracks.length : 0, buses ? buses.length : 0) : null
  const window = checkLimiter(limiterAsked, opts.limiterWindow, loud.target, sampleRate) // (the limiter's window in samples, 0 without one)
  const release = checkLimiterRelease(opts.limiterRelease, limiterAsked, sampleRate) // (... and its release, 0 without one)
  if (meters && !(sampleRate >= 8000)) throw METER_RATE_LOW(sampleRate)
  const nBlocks = meterBlocks(nSamples, sampleRate)
  const idle = { engaged: false, threshold: 0, window, reduction: 1, lufsIn: -Infinity, truePeakIn: 0, release } // (a timeline of no samples)
  const delivered = loud.target !== null ? (got) => Object.assign({ gain: got ? got.gain : 1, level: got ? got.level : 1 }, window ? { limiter: got ? got.limiter : idle } : {}) : () => null
  if (nSamples === 0) return { nSamples, nChannels, sampleRate, result: null, names, metered: meters ? metersOf(names || ['mix'], null, nChannels, 0, sampleRate, truePeaks) : null, loud: delivered(null) }
  const progs = [], busProgs = [], trackProgs = []
  let masterProg = null
  try {
    for (const part of grouped.parts) progs.push(n.programBuild(contextFor(sampleRate), part.uni.words, engine))
    if (master) masterProg = n.programBuild(contextFor(sampleRate), master.words, engine)
    if (buses) for (const bus of buses) busProgs.push(n.programBuild(contextFor(sampleRate), bus.words, engine))
    const args = [progs, Float64Array.from(grouped.parts, (part) => part.uni.nInstances), Float64Array.from(grouped.parts, (part) => part.nVoiceSamples),
      grouped.parts.map((part) => (part.uni.nParams ? part.uni.params : null)), grouped.partOf, onsets, lengths, g, nSamples, tileBytes, format, normalise]
    if (groups) for (const group of groups) trackProgs.push(n.programBuild(contextFor(sampleRate), group.uni.words, engine))
    const result = meters ? await (release ? n.renderPieceLimiterRelease : window ? n.renderPieceLimiter : truePeaks ? n.renderPieceLoudness : n.renderPieceMeters)(...args, stereo ? 3 : taps ? 2 : panned ? 1 : 0, fracs, panned ? panned.pans : null, panned ? panned.comp : null,
      taps ? taps.nSpeakers : 0, taps ? taps.delays : null, taps ? taps.gains : null, masterProg, master && master.nParams ? master.params : null,
      buses ? busProgs : null, buses ? buses.map((bus) => (bus.nParams ? bus.params : null)) : null, routed ? null : sends, routed ? opts.tracks.length : 0, routed ? routed.trackOf : null,
      routed ? trackProgs : null, routed ? groups.map((group) => Uint32Array.from(group.tracks)) : null, routed ? groups.map((group) => (group.uni.nParams ? group.uni.params : null)) : null,
      routed ? routed.faders : null, routed ? routed.trackSends : null, stems, nBlocks, ...(truePeaks ? [loud.target !== null, loud.target === null ? 0 : loud.target, loud.ceiling] : []), ...(window ? [window] : []), ...(release ? [release] : []))
      : stems ? await n.renderPieceStems(...args, stereo ? 3 : taps ? 2 : panned ? 1 : 0, fracs, panned ? panned.pans : null, panned ? panned.comp : null,
      taps ? taps.nSpeakers : 0, taps ? taps.delays : null, taps ? taps.gains : null, masterProg, master && master.nParams ? master.params : null,
      buses ? busProgs : null, buses ? buses.map((bus) => (bus.nParams ? bus.params : null)) : null, routed ? null : sends, routed ? opts.tracks.length : 0, routed ? routed.trackOf : null,
      routed ? trackProgs : null, routed ? groups.map((group) => Uint32Array.from(group.tracks)) : null, routed ? groups.map((group) => (group.uni.nParams ? group.uni.params : null)) : null,
      routed ? routed.faders : null, routed ? routed.trackSends : null)
      : routed ? await n.renderPieceTracks(...args, stereo ? 3 : taps ? 2 : panned ? 1 : 0, fracs, panned ? panned.pans : null, panned ? panned.comp : null,
      taps ? taps.nSpeakers : 0, taps ? taps.delays : null, taps ? taps.gains : null, masterProg, master && master.nParams ? master.params : null,
      buses ? busProgs : null, buses ? buses.map((bus) => (bus.nParams ? bus.params : null)) : null, null, opts.tracks.length, routed.trackOf, trackProgs,
      groups.map((group) => Uint32Array.from(group.tracks)), groups.map((group) => (group.uni.nParams ? group.uni.params : null)), routed.faders, routed.trackSends)
      : buses ? await n.renderPieceBuses(...args, panned ? 1 : 0, null, panned ? panned.pans : null, panned ? panned.comp : null, 0, null, null,
      masterProg, master && master.nParams ? master.params : null, busProgs, buses.map((bus) => (bus.nParams ? bus.params : null)), sends)
      : master ? await n.renderPieceMaster(...args, stereo ? 3 : taps ? 2 : panned ? 1 : 0, fracs, panned ? panned.pans : null, panned ? panned.comp : null,
      taps ? taps.nSpeakers : 0, taps ? taps.delays : null, taps ? taps.gains : null, masterProg, master.nParams ? master.params : null)
      : stereo ? await n.renderPieceStereo(...args, fracs, panned.pans, panned.comp)
      : taps ? await n.renderPieceSpace(...args, taps.nSpeakers, taps.delays, taps.gains)
      : fracs ? await n.renderPieceFrac(...args, fracs, panned ? panned.pans : null, panned ? panned.comp : null)
      : panned ? await n.renderPiecePan(...args, panned.pans, panned.comp) : await n.renderPiece(...args)
    if (!meters) return { nSamples, nChannels, sampleRate, result, names }
    // (one addon call: { data, peaks, rms, lufs, momentary }; without stems what is delivered is the call's without meters)
    return { nSamples, nChannels, sampleRate, result: stems || format ? result : result.data, names, metered: metersOf(names || ['mix'], result, nChannels, nBlocks, sampleRate, truePeaks), loud: delivered(result) }
  } finally {
    for (const prog of progs) n.programDestroy(prog)
    if (masterProg) n.programDestroy(masterProg)
    for (const prog of busProgs) n.programDestroy(prog)
    for (const prog of trackProgs) n.programDestroy(prog)
  }
}

/* A PIECE of several instruments: renderScore over voices of ANY circuits, each rendered for its own voiceDurations[k] seconds (one
 * number: all alike).  The voices are grouped into parts by structure and by samples a voice (pieceParts), every part is ONE program,
 * and the device walks the caller's voice list in its own order (dusp_render_host_score_parts): what
 * renderChannelData(Sum.many(outlets.map((v, k) => new Delay(v, onsets[k], maxDelay))), duration) computes, however the instruments
 * interleave.  Voices whose circuits differ in output channels are refused before anything is built.  onsets, lengths (within the
 * voice's own samples), gains and engine as renderScore; tileBytes: what a tile of voices may take on the device (0: the default).
 * pans (one finite number a voice, -1 left .. +1 right, not clamped): the voices are MONO circuits and voice k is placed in the stereo
 * field where it is added to the timeline (dusp_render_host_score_parts_pan) — what the reference renders for new Pan(voice_k, pans[k])
 * in the voice's place, bit for bit, the compensation being this engine's own Math.pow.  The result has two channels.
 * fracs (one number a voice, 0 <= f < 1; onsets stay whole numbers): voice k starts at onsets[k] + fracs[k] samples — what the reference
 * renders for new Delay(., onsets[k] + fracs[k], maxDelay), whose two taps carry the weights 1 - frac and frac
 * (dusp_render_host_score_parts_frac; include/dusp_hip.h says where the reference's ring departs from it).  splitOnsets makes both
 * arrays from positions in samples written as real numbers.  All fractions zero gives the bits of the call without.
 * places (one position a voice, 1 to 3 coordinates in metres), with speakers (default [[-1, 0], [1, 0]]; 1 to 8, the same number of
 * coordinates), decibelsPerMetre (-3) and sampleDelayPerMetre (sample rate / 343): the voices are MONO circuits and every speaker — a
 * channel of the result — hears voice k attenuated and delayed by its distance, what the reference's Space patch does behind a sound
 * (dusp_render_host_score_parts_space; spaceTaps makes the gain and the delay per voice and speaker; include/dusp_hip.h says where
 * the reference's own wiring departs from it).  Not together with pans or fracs.
 * stereo: true — a voice may be a MONO circuit or one of TWO channels, side by side, and the result has two channels
 * (dusp_render_host_score_parts_stereo).  pans may be left out (nothing is placed) or hold null / NaN for a voice that is not placed: a
 * mono voice with a pan is the panned voice above, a mono voice without one is heard alike on both channels (the reference's Sum reads
 * a mono input for every channel of a wider one), a voice of two channels keeps its channels and takes no pan (the Pan unit's inlet is
 * mono).  What the reference renders for Sum.many over such voices behind their Delays, bit for bit.  fracs work as above; places are
 * refused.  Without the option every call is what it was.
 * master: the mix through a circuit before it is delivered — an EQ, an echo, a comb or all-pass, a clip on the sum — on the device,
 * whatever the placement (dusp_render_host_score_piece).  A function fx(x), given a fresh MasterInput once per channel of the timeline
 * and returning a MONO circuit over it, or an array of one function a channel; the circuits are isomorphic and may differ in constants
 * (masterProgram).  Channel c of the result is the render of the master over the timeline's channel c as the chain left it — before
 * `|| 0`, as a unit behind Sum.many hears it — from the master's initial state (DESIGN.md 6.14 says where that is the reference's
 * fx(Sum.many(...)) bit for bit and where it is not).  The call's engine is the master's too.
 * buses, sends: effect sends — some notes, at a level of their own, into an effect such as an echo, and its return beside the dry mix
 * (dusp_render_host_score_piece_buses; DESIGN.md 6.15).  buses: an array of 1 .. 4 circuits, each given as a master is; sends: an array
 * of one array of levels a bus (one bus: the levels themselves will do), sends[b][k] what voice k gives to bus b.  Bus b hears the chain
 * of every voice's dry term — after its gain and its pan — times its level, is rendered over that timeline as a master is over the mix,
 * and the buses' outputs are added to the dry mix in order, in front of the master where there is one.  A level of 0 is a
 * multiplication by 0, not a voice left out.  With plain voices and with pans; fracs, places and stereo are refused with sends.
 * tracks, trackOf, faders, trackSends: sub-mixes — some of the voices through a circuit of their own before they reach the mix
 * (dusp_render_host_score_piece_tracks; DESIGN.md 6.16).  tracks: an array of 1 .. 8 entries, each given as a master is or null for a
 * track without a circuit, a fader group; trackOf: one whole number a voice, the track it goes to or -1 for straight to the mix.  Track
 * g hears the chain of ITS voices — the call's placement over them alone, raw — and is rendered over it as a master is over the mix;
 * tracks with isomorphic circuits are ONE program (trackPrograms).  faders (one finite number a track) scale the tracks' outputs, which
 * are added to the direct voices' chain in order; with buses, trackSends[b][g] is what track g gives to bus b, and sends is refused.
 * Whatever the placement, with or without a master.
 * stems: true — the call resolves to its stems beside the mix (dusp_render_host_score_piece_stems; DESIGN.md 6.17; stemsOf says what
 * it holds): the direct mix (with tracks the voices that go straight to the mix, else the dry mix of all voices), every track after
 * its fader and every bus's return, each as the mix is delivered, and the mix itself, bit for bit the call's result without stems.  The
 * stems are taken in front of the master; without a master they add up to the mix.  Every signal has its peak, and PCM frames get ONE
 * gain from the largest of them.  One addon call, one delivery.  What is no boolean is refused.
 * meters: true — the call also meters what it delivers, on the device, in front of the PCM gain (dusp_render_host_score_piece_meters;
 * DESIGN.md 6.18; metersOf says what `meters` holds): the RMS a channel, the gated integrated loudness in LUFS (ITU-R BS.1770-4) and the
 * momentary loudness of every 400 ms block, of the mix and — with stems — of every stem.  With stems the result gains `.meters`; without,
 * the call resolves to { mix, meters }, mix what it resolves to without meters bit for bit.  One addon call.  What is no boolean is
 * refused, next to stems.
 * truePeak: true (implies meters) — `meters.truePeak`, name -> Float64Array [channels]: the true peak of every channel of every delivered
 * signal, oversampled on the device (dusp_render_host_score_piece_loudness; DESIGN.md 6.19), linear: dBTP is 20 log10.
 * loudness, truePeakMax (renderPiecePcm and renderPieceWav; here loudness is refused): the target in LUFS and the ceiling in dBTP
 * (default -1): the frames of every signal are encoded under ONE gain that brings the mix to the target, lowered where the largest true
 * peak of any signal would exceed the ceiling.  The result gains `gain` and `level`; every `peak` stays the sample peak.  Not together
 * with normalise != 0. */
async function renderPiece(outlets, opts = {}) {
  const { nSamples, nChannels, sampleRate, result, names, metered } = await pieceCall('renderPiece', outlets, opts, 0, 0)
  if (names) return withMeters(planarStems(names, nSamples, nChannels, sampleRate, result), metered)
  const channelData = []
  channelData.sampleRate = sampleRate
  if (result) for (let c = 0; c < nChannels; c++) channelData.push(result.subarray(c * nSamples, (c + 1) * nSamples))
  return withMeters(channelData, metered)
}

async function renderPiecePcm(outlets, opts = {}) {
  const { bitDepth = 16, normalise = 0 } = opts
  if (bitDepth !== 16 && bitDepth !== 24 && bitDepth !== 32) throw 'dusp-hip: renderPiecePcm: bitDepth must be 16, 24 or 32'
  if (normalise !== 0 && normalise !== 1 && normalise !== 2) throw 'dusp-hip: renderPiecePcm: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale)'
  const { nChannels, sampleRate, result, names, metered, loud } = await pieceCall('renderPiecePcm', outlets, opts, PCM_FORMAT[bitDepth], normalise)
  if (names) return withMeters(pcmStems(names, nChannels, sampleRate, result, bitDepth, normalise), metered, loud)
  if (!result) return withMeters({ data: Buffer.alloc(0), bitDepth, numberOfChannels: 0, sampleRate, peak: 0 }, metered, loud)
  return withMeters({ data: result.data, bitDepth, numberOfChannels: nChannels, sampleRate, peak: result.peaks[0] }, metered, loud)
}

async function renderPieceWav(outlets, opts = {}) {
  return wavOf(await renderPiecePcm(outlets, opts))
}

/* A flat descriptor (what lib/extract.js produces — from this package's graph classes or from the reference's own objects,
 * patches included: their units reach the extractor as they are) rendered as it stands: no host objects, hence no events,
 * no host-ticked units, no state write-back.  Resolves to channelData like renderChannelData. */
async function renderDescriptor(words, nSamples, { engine = 0 } = {}) {
  const sampleRate = words[2]
  const n = native()
  const prog = n.programBuild(contextFor(sampleRate), words, engine)
  try {
    const info = n.programInfo(prog)
    const pcm = await n.render(prog, 1, nSamples, null)
    const channelData = []
    for (let c = 0; c < info.nOutChannels; c++) channelData.push(pcm.subarray(c * nSamples, (c + 1) * nSamples))
    channelData.sampleRate = sampleRate
    return channelData
  } finally {
    n.programDestroy(prog)
  }
}

module.exports = renderChannelData
module.exports.renderChannelData = renderChannelData
module.exports.renderDescriptor = renderDescriptor
module.exports.renderMany = renderMany
module.exports.renderPcm = renderPcm
module.exports.renderWav = renderWav
module.exports.renderMix = renderMix
module.exports.renderMixPcm = renderMixPcm
module.exports.renderMixWav = renderMixWav
module.exports.renderScore = renderScore
module.exports.renderScorePcm = renderScorePcm
module.exports.renderScoreWav = renderScoreWav
module.exports.renderPiece = renderPiece
module.exports.renderPiecePcm = renderPiecePcm
module.exports.renderPieceWav = renderPieceWav
module.exports.pieceParts = pieceParts
module.exports.structureKey = structureKey
module.exports.checkPieceChannels = checkPieceChannels
module.exports.checkPanChannels = checkPanChannels
module.exports.panArrays = panArrays
module.exports.stereoPanArrays = stereoPanArrays
module.exports.checkStereoKinds = checkStereoKinds
module.exports.fracArrays = fracArrays
module.exports.splitOnsets = splitOnsets
module.exports.spaceTaps = spaceTaps
module.exports.checkPlaces = checkPlaces
module.exports.checkSpaceChannels = checkSpaceChannels
module.exports.masterProgram = masterProgram
module.exports.MASTER = MASTER
module.exports.BUS = BUS
module.exports.SENDS = SENDS
module.exports.checkSends = checkSends
module.exports.TRACK = TRACK
module.exports.TRACKS = TRACKS
module.exports.checkTracks = checkTracks
module.exports.trackPrograms = trackPrograms
module.exports.STEMS_NOT_BOOL = STEMS_NOT_BOOL
module.exports.stemNames = stemNames
module.exports.commonPeak = commonPeak
module.exports.METERS_NOT_BOOL = METERS_NOT_BOOL
module.exports.METER_RATE_LOW = METER_RATE_LOW
module.exports.meterHop = meterHop
module.exports.meterBlocks = meterBlocks
module.exports.meter = meter
module.exports.truePeak = truePeak
module.exports.limit = limit
module.exports.LIMITER = LIMITER
module.exports.checkLimiter = checkLimiter
module.exports.checkLimiterRelease = checkLimiterRelease
module.exports.TRUE_PEAK_NOT_BOOL = TRUE_PEAK_NOT_BOOL
module.exports.LOUDNESS = LOUDNESS
module.exports.instanceRange = instanceRange
module.exports.deviceCount = () => native().deviceCount()
module.exports.SegmentRenderer = SegmentRenderer
