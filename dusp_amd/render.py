"""`renderChannelData(outlet, duration)` — the drop-in surface of the render path
(reference src/renderChannelData.js:5-49), executed on the MI355X.

    channelData = renderChannelData(unit_or_outlet, duration)
    channelData[c]          -> numpy float32 array of duration*sampleRate samples
    channelData.sampleRate  -> like the reference's expando (renderChannelData.js:47)

plus the batched form the reference cannot express: `render_many(outlets, duration)`
renders N structurally identical circuits (voices, a parameter sweep) as ONE
program with a per-instance parameter table.
"""
import numpy as np

from . import descriptor, mix, runtime, wav
from .mix import check_pan_channels, check_piece_channels, check_space_channels, check_stereo_channels  # noqa: F401 (what a piece's parts are held to)

_contexts = {}


def context(sample_rate, device=-1):
    key = (device, sample_rate)
    if key not in _contexts:
        _contexts[key] = runtime.Context(device, sample_rate)
    return _contexts[key]


class ChannelData(list):
    """Array of per-channel sample arrays with a `.sampleRate`, as the reference returns."""
    sampleRate = None


def _n_samples(duration, sample_rate):
    n = int(duration * sample_rate)  # `new TypedArray(lengthInSamples)` truncates (renderChannelData.js:24,39)
    if n < 0:
        raise descriptor.DuspError("negative duration")
    return n


def write_back(prog, circuit, chunk_size, n_samples, instance=0):
    """Leave the unit objects as the reference leaves them after ticking ceil(n_samples/chunk) chunks: state
    fields from the device (dusp_state_download), circuit.clock advanced (twin of renderChannelData.js writeBack)."""
    D = descriptor
    for u, unit in enumerate(circuit.units):
        op = D.UNITS[type(unit).__name__][0]
        if op in (D.OP_OSC,):
            unit.phase = float(prog.state(u, instance)[0])
        elif op == D.OP_RAMP:
            st = prog.state(u, instance)
            unit.t, unit.playing = float(st[0]), bool(st[1])
        elif op in (D.OP_CB_READER, D.OP_CB_WRITER, D.OP_TIMER):
            unit.t = float(prog.state(u, instance)[0])
        elif op in (D.OP_FIXED_DELAY, D.OP_COMB_FILTER, D.OP_ALL_PASS, D.OP_READBACK_DELAY):
            unit.tBuffer = float(prog.state(u, instance)[0])
        elif op == D.OP_MULTI_OSC:
            st = prog.state(u, instance)
            unit.phase = [float(v) for v in st[1:1 + int(st[0])]]
        elif op == D.OP_FILTER:
            st = prog.state(u, instance)
            if st[0]:
                unit.lastF = float(st[1])
            unit.a0, unit.a1, unit.a2, unit.b1, unit.b2 = (float(v) for v in st[2:7])
            nch = int(st[7])
            hist = st[8:8 + 4 * nch].reshape(nch, 4)
            unit.x1, unit.x2, unit.y1, unit.y2 = ([float(v) for v in hist[:, k]] for k in range(4))
        elif op == D.OP_SHAPE:
            st = prog.state(u, instance)
            unit.t, unit.playing, unit.finished = float(st[0]), bool(st[1]), bool(st[2])
        elif op == D.OP_AHD:
            st = prog.state(u, instance)
            unit.state, unit.playing, unit.t = int(st[0]), bool(st[1]), float(st[2])
        elif op == D.OP_SAMPLE_RATE_REDUX:
            st = prog.state(u, instance)
            unit.timeSinceLastUpdate = float(st[0])
            unit.val = [float(v) for v in st[2:2 + int(st[1])]]
    circuit.clock += ((n_samples + chunk_size - 1) // chunk_size) * chunk_size


def _no_master_input(extraction):
    """a circuit rendered by itself holds no MasterInput: that unit stands for the timeline of a score or piece (refused before a device is asked for)"""
    if any(getattr(src, "isMasterInput", False) for src in extraction.sources):
        raise descriptor.DuspError(mix.MASTER_INPUT_ALONE)
    return extraction


def _host_inputs(sources, clock, length):
    """This segment's samples of the circuit's HostSource units -> float32 [n_sources, 1, length] (zeros past a source's end)."""
    if not sources:
        return None
    block = np.zeros((len(sources), 1, length), dtype=np.float32)
    for k, src in enumerate(sources):
        have = src.samples[clock:clock + length]
        block[k, 0, :have.size] = have
    return block


def renderChannelData(outlet, duration=1, TypedArray=np.float32, engine=runtime.ENGINE_AUTO, device=-1):
    """Drop-in for reference src/renderChannelData.js:5-49.  Scheduled events (unit.schedule / scheduleTrigger) are
    honoured the way the reference's Circuit.tick does (Circuit.js:23,57-65): every event due before the end of a
    chunk runs on the host objects before that chunk is rendered; the render is segmented at those boundaries and
    ONE device program is continued from segment to segment (dusp_program_continue), so delay lines, CircleBuffers
    and feedback chunks stay resident on the device.  Afterwards the circuit is consumed like the reference's:
    circuit.clock has advanced and the unit objects hold their post-render state."""
    return _render_extracted(outlet, _no_master_input(descriptor.extract(outlet, allow_events=True)), duration, TypedArray, engine, device)


def _render_extracted(outlet, first, duration, TypedArray, engine, device):
    circuit, chunk = first.circuit, first.chunk_size
    n = _n_samples(duration, first.sample_rate)
    result = ChannelData()
    result.sampleRate = first.sample_rate
    if n == 0:
        return result
    has_events = bool(circuit.events)
    ctx = context(first.sample_rate, device)
    end = ((n + chunk - 1) // chunk) * chunk
    prog, clock, segments = None, 0, []
    try:
        while clock < end:
            nxt = end
            if has_events:
                circuit.runEvents(clock + chunk)
                if circuit.events:
                    due = int(circuit.events[0].t // chunk) * chunk
                    nxt = min(end, max(clock + chunk, due))
            ex = first if (clock == 0 and not has_events) else descriptor.extract(outlet, allow_events=True, allow_clock=True)
            if prog is None:
                prog = ctx.build(ex.words, engine | runtime.ENGINE_RESUMABLE if has_events else engine)
            else:
                prog.continue_with(ex.words)
            length = min(nxt, n) - clock  # the last segment may end inside a chunk
            segments.append(prog.render(length, 1, inputs=_host_inputs(ex.sources, clock, length))[0])
            write_back(prog, circuit, chunk, length)  # advances circuit.clock to `nxt`
            clock = nxt
    finally:
        if prog is not None:
            prog.close()
    n_channels = max(seg.shape[0] for seg in segments)
    pcm = np.zeros((n_channels, n), dtype=np.float32)  # late channels start as zeros (renderChannelData.js:38-39)
    at = 0
    for seg in segments:
        pcm[:seg.shape[0], at:at + seg.shape[1]] = seg
        at += seg.shape[1]
    for c in range(n_channels):
        result.append(pcm[c].astype(TypedArray, copy=False))
    return result


def render_many(outlets, duration=1, engine=runtime.ENGINE_AUTO, device=-1):
    """Render N isomorphic circuits at once -> float32 [N, n_channels, n_samples]."""
    uni = descriptor.unify([descriptor.extract(o) for o in outlets])
    n = _n_samples(duration, uni.sample_rate)
    prog = context(uni.sample_rate, device).build(uni.words, engine)
    try:
        return prog.render(n, uni.n_instances, uni.params)
    finally:
        prog.close()


def _mix_program(outlets, duration, engine, device):
    uni = descriptor.unify([descriptor.extract(o) for o in outlets])
    return uni, _n_samples(duration, uni.sample_rate), context(uni.sample_rate, device).build(uni.words, engine)


def render_mix(outlets, duration=1, gains=None, engine=runtime.ENGINE_AUTO, device=-1, tile_instances=0):
    """The mix of N isomorphic circuits — what `renderChannelData(Sum.many(outlets), duration)` computes (Sum.js:18-29: a left-deep chain,
    one f32 rounding per add), with `gains` what Sum.many of Multiply(outlet, g_i) does — rendered as ONE program in tiles and summed on the
    device in that order (Program.render_mix): memory is bounded by the tile, not by N, and one voice's worth of samples is downloaded.
    A voice sample that is NaN drops that voice out of the sample (the reference's Sum would zero the whole mix sample there)."""
    return _render_mix(outlets, duration, gains, engine, device, tile_instances)


def _check_pcm(bit_depth, normalise):
    if bit_depth not in _PCM_FORMAT:
        raise descriptor.DuspError("dusp-hip: bit depth must be 16, 24 or 32")
    if normalise not in (0, 1, 2):
        raise descriptor.DuspError("dusp-hip: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale)")


def _wav(pcm, bit_depth):
    """PcmData -> a complete RIFF/WAVE file (bytes); a Stems of PcmData -> a Stems of files"""
    if isinstance(pcm, Stems):
        return pcm.each(lambda one: _wav(one, bit_depth))
    if isinstance(pcm, Metered):
        return Metered(_wav(pcm.mix, bit_depth), pcm.meters, getattr(pcm, "gain", None), getattr(pcm, "level", None), getattr(pcm, "limiter", None))
    if bit_depth == 32:
        return wav.encode_wav(pcm.data, pcm.sampleRate, 32, frames=True)
    return wav.encode_wav(pcm.data, pcm.sampleRate, bit_depth)


def _delivered(pcm, sample_rate, n, channels, run):
    """What a mix, score or piece hands back.  pcm None: ChannelData of what run(None, 0) renders; pcm (bit_depth, normalise): PcmData
    of the frames and the peak that run(format, normalise) renders.  A timeline of no samples (n == 0) renders nothing: an empty
    ChannelData, or frames of no samples (of `channels` channels)."""
    if pcm is None:
        result = ChannelData()
        result.sampleRate = sample_rate
        if n > 0:
            result.extend(run(None, 0))
        return result
    bit_depth, normalise = pcm
    if n == 0:
        data, peak = wav.encode_frames(np.zeros((channels, 0), dtype=np.float32), bit_depth, normalise)
    else:
        data, peak = run(_PCM_FORMAT[bit_depth], normalise)
    return PcmData(data, bit_depth, sample_rate, peak)


class Stems:
    """What a score or piece call with stems=True hands back (mix.stems is the contract): `names`, the signals in the
    order they were delivered (mix.stem_names: direct, track0 .., bus0 .., mix); `mix`, exactly what the call returns without stems;
    `direct`, `tracks` (a list, one a track) and `buses` (a list, one a bus), each of the mix's type — ChannelData, PcmData, or the
    bytes of a WAV file; `peaks`, name -> numpy.float32, every signal's own max |x| over all its channels; `peak`, the largest of them
    (wav.common_peak); and for PCM `gain`, the one gain all the frames were encoded under (wav.gain(peak, normalise)) — with loudness=
    the gain of mix.loudness_gain, and `level` beside it; with limiter=True `limiter`, a Limiter, and everything describes the limited
    signals."""

    def __init__(self, names, signals, peaks, gain=None):
        self.names, self._signals = list(names), list(signals)
        n_tracks = sum(1 for name in self.names if name.startswith("track"))
        self.direct, self.tracks, self.buses, self.mix = self._signals[0], self._signals[1:1 + n_tracks], self._signals[1 + n_tracks:-1], self._signals[-1]
        self.peaks = {name: np.float32(p) for name, p in zip(self.names, peaks)}
        self.peak = wav.common_peak(np.asarray(peaks, dtype=np.float32))
        if gain is not None:
            self.gain = gain

    def __getitem__(self, name):
        return self._signals[self.names.index(name)]

    def each(self, make):
        """the same Stems with make(signal) for every signal"""
        made = Stems(self.names, [make(one) for one in self._signals], [self.peaks[name] for name in self.names], getattr(self, "gain", None))
        for extra in ("meters", "level", "limiter"):
            if hasattr(self, extra):
                setattr(made, extra, getattr(self, extra))
        return made


class Meters:
    """The meters of a call with meters=True (mix.meters is the contract), taken on the f32 signals in front of the PCM
    gain: `names`, the signals in the order they were delivered (mix.stem_names with stems, else ["mix"]); `rms`, name -> float64
    [channels]; `lufs`, name -> float, the gated integrated loudness of ITU-R BS.1770-4 (-inf: no block above the gates, NaN: a sample
    that is not finite); `momentary`, name -> float64 [n_blocks], the loudness of every 400 ms block, 100 ms apart; `hop` and `block`
    in samples.  The loudness of an encoded file is lufs + 20 log10(gain).  With true_peak=True (or loudness=): `true_peak`, name ->
    float64 [channels], the true peak of every channel (mix.true_peak is the contract), LINEAR: dBTP is 20 log10."""

    def __init__(self, names, got):
        self.names = list(names)
        self.rms = {name: np.array(got["rms"][k], dtype=np.float64) for k, name in enumerate(self.names)}
        self.lufs = {name: float(got["lufs"][k]) for k, name in enumerate(self.names)}
        self.momentary = {name: np.array(got["momentary"][k], dtype=np.float64) for k, name in enumerate(self.names)}
        self.hop, self.block = int(got["hop"]), int(got["block"])
        if "true_peak" in got:
            self.true_peak = {name: np.array(got["true_peak"][k], dtype=np.float64) for k, name in enumerate(self.names)}


class Metered:
    """What a score or piece call with meters=True and without stems hands back: `mix`, exactly what the call returns without meters,
    and `meters`, a Meters of the one signal "mix".  A call with loudness= adds `gain`, the gain the frames were encoded under, and
    `level`, the numpy.float32 sample magnitude that was brought to full scale (mix.loudness_gain); `mix.peak` stays the sample peak.
    A call with limiter=True adds `limiter`, a Limiter; where it engaged, the meters, the peak, gain and level are the limited mix's."""

    def __init__(self, mix_, meters, gain=None, level=None, limiter=None):
        self.mix, self.meters = mix_, meters
        if gain is not None:
            self.gain, self.level = gain, level
        if limiter is not None:
            self.limiter = limiter


class Limiter:
    """What the limiter of a call with limiter=True did (mix.deliver_limited is the contract): `engaged`, whether it ran —
    it does where the largest true peak lies above `threshold`, the ceiling seen from the loudness target, linear; `window`, its
    look-ahead, attack and release in samples; `reduction`, the smallest gain of its curve, 1.0 when not engaged; `lufs_in` and
    `true_peak_in`, the loudness of the mix and the largest true peak of any delivered signal in front of it; `release`, the release of
    its own in samples (limiter_release=), 0 when there is none and the curve leaves a peak within `window`."""

    def __init__(self, got):
        self.engaged, self.threshold, self.window, self.reduction = bool(got["engaged"]), float(got["threshold"]), int(got["window"]), float(got["reduction"])
        self.lufs_in, self.true_peak_in = float(got["lufs_in"]), float(got["true_peak_in"])
        self.release = int(got.get("release", 0))


def limit(planar, sample_rate, threshold, window, release=None, device=-1):
    """The linked look-ahead limiter over any signals a user has: planar float32 [signals, channels, samples] (or [channels, samples]:
    one signal) -> (limited float32 of that shape, g float64 [samples], reduction), ONE gain curve for every row, on the device
    (Context.limit; mix.limit is the contract).  threshold: linear; window: 1 .. 4096 samples; release: None, or the limiter's release
    of its own, 1 .. 2^22 samples (mix.limiter_gain_release)."""
    return context(sample_rate, device).limit(planar, sample_rate, threshold, window, 0 if release is None else release)


def _empty_meters(n_signals, channels, sample_rate):
    """the meters of a timeline of no samples, which renders nothing: no energy, no block"""
    if not sample_rate >= mix.METER_RATE_MIN:
        raise ValueError(mix.METER_RATE_LOW % sample_rate)
    hop = mix.meter_hop(sample_rate)
    return dict(rms=np.zeros((n_signals, channels)), lufs=np.full(n_signals, -np.inf), momentary=np.zeros((n_signals, 0)), hop=hop, block=4 * hop)


def meter(planar, sample_rate, device=-1):
    """The meters of any signals a user has: planar float32 [signals, channels, samples] (or [channels, samples]: one signal) -> a
    Meters whose names are "0", "1", ..., metered on the device and gated in the library (Context.meter; mix.meters is the contract)."""
    got = context(sample_rate, device).meter(planar, sample_rate)
    return Meters([str(k) for k in range(len(got["lufs"]))], got)


def true_peak(planar, sample_rate, device=-1):
    """The true peak of any signals a user has: planar float32 [signals, channels, samples] (or [channels, samples]: one signal) ->
    float64 [signals, channels], linear (dBTP is 20 log10), taken on the device (Context.true_peak; mix.true_peak is the contract)."""
    return context(sample_rate, device).true_peak(planar, sample_rate)


def _delivered_stems(pcm, sample_rate, n, channels, names, run):
    """_delivered for a call with stems: run(format, normalise) -> (signals [S + 1, ...], peaks [S + 1]) -> Stems"""
    def channel_data(planar):
        result = ChannelData()
        result.sampleRate = sample_rate
        result.extend(planar)
        return result

    if pcm is None:
        if n == 0:
            return Stems(names, [channel_data([]) for _ in names], np.zeros(len(names), dtype=np.float32))
        signals, peaks = run(None, 0)
        return Stems(names, [channel_data(one) for one in signals], peaks)
    bit_depth, normalise = pcm
    if n == 0:
        signals, peaks = wav.encode_stems(np.zeros((len(names), channels, 0), dtype=np.float32), bit_depth, normalise)
    else:
        signals, peaks = run(_PCM_FORMAT[bit_depth], normalise)
    return Stems(names, [PcmData(one, bit_depth, sample_rate, p) for one, p in zip(signals, peaks)], peaks, wav.gain(wav.common_peak(peaks), normalise))


def _render_mix(outlets, duration, gains, engine, device, tile_instances, pcm=None):
    """render_mix (pcm None) and render_mix_pcm (pcm = (bit_depth, normalise))"""
    if pcm is not None:
        _check_pcm(*pcm)
    uni, n, prog = _mix_program(outlets, duration, engine, device)
    try:
        return _delivered(pcm, uni.sample_rate, n, prog.n_out_channels,
                          lambda format, normalise: prog.render_mix(n, uni.n_instances, uni.params, gains, tile_instances, format, normalise))
    finally:
        prog.close()


def render_mix_pcm(outlets, duration=1, bit_depth=16, normalise=0, gains=None, engine=runtime.ENGINE_AUTO, device=-1, tile_instances=0):
    """render_mix, delivering what render_pcm delivers: the mix's frames encoded on the device, and its peak -> PcmData."""
    return _render_mix(outlets, duration, gains, engine, device, tile_instances, (bit_depth, normalise))


def render_mix_wav(outlets, duration=1, bit_depth=16, normalise=0, gains=None, engine=runtime.ENGINE_AUTO, device=-1, tile_instances=0):
    """A complete RIFF/WAVE file (bytes) of the mix: render_mix_pcm plus the header (wav.encode_wav)."""
    return _wav(render_mix_pcm(outlets, duration, bit_depth, normalise, gains, engine, device, tile_instances), bit_depth)


def _voice_arrays(onsets, lengths, gains, n, samples, noun, within):
    """onsets, lengths and gains of n voices, checked -> int64, int64 or None, float32 or None.  samples: the most a length may be, one
    number or one a voice; noun and within: the caller's words for the gains' shape and for where lengths must lie."""
    onsets = runtime._whole_samples(onsets, n, "onsets")
    if lengths is not None:
        lengths = runtime._whole_samples(lengths, n, "lengths")
        if np.any(lengths < 0) or np.any(lengths > samples):
            raise ValueError("dusp-hip: lengths must lie in 0 .. " + within)
    return onsets, lengths, runtime._gains_table(gains, n, noun)


def _score_program(outlets, onsets, voice_duration, duration, lengths, gains, engine, device):
    """-> unified voices, samples a voice, samples of timeline, onsets, lengths, gains (checked, whatever the durations), program"""
    uni = descriptor.unify([descriptor.extract(o) for o in outlets])
    n_voice, n_total = _n_samples(voice_duration, uni.sample_rate), _n_samples(duration, uni.sample_rate)
    if n_voice == 0:
        raise descriptor.DuspError("dusp-hip: voice_duration must cover at least one sample")
    onsets, lengths, gains = _voice_arrays(onsets, lengths, gains, uni.n_instances, n_voice, "n_instances", "the voice's %d samples" % n_voice)
    return uni, n_voice, n_total, onsets, lengths, gains, context(uni.sample_rate, device).build(uni.words, engine)


def _score_voice_duration(voice_duration):
    """render_score with pans or fracs goes through the piece's call as ONE part: one duration for all voices"""
    if np.ndim(voice_duration) != 0:
        raise ValueError("dusp-hip: voice_duration is one number")
    return voice_duration


def render_score(outlets, onsets, voice_duration=1, duration=1, lengths=None, gains=None, engine=runtime.ENGINE_AUTO, device=-1, tile_instances=0, pans=None, fracs=None, places=None, speakers=None, decibels_per_metre=-3, sample_delay_per_metre=None, stereo=False, master=None, buses=None, sends=None, tracks=None, track_of=None, faders=None, track_sends=None, stems=False, meters=False, true_peak=False, loudness=None, limiter=False, limiter_window=0.005, limiter_release=None):
    """A piece of N isomorphic circuits, voice k starting at sample onsets[k] of a timeline of `duration` seconds — what
    `renderChannelData(Sum.many(Delay(outlet_k, onsets[k], maxDelay)), duration)` computes (a Delay by whole samples is its input behind
    zeros; the voice with onset 0 bare), with `gains` as in render_mix — rendered as ONE program for `voice_duration` seconds a voice, in
    tiles, and mixed on the device at the onsets (Program.render_score; mix.score_chain is the contract).  onsets and lengths are in
    SAMPLES, whole numbers of any sign (lengths clip a voice to its first len_k samples); the durations are in seconds.  A voice_duration
    of no samples is refused, and onsets, lengths and gains are checked whatever the durations.

    pans: as render_piece's — mono voices, two channels out; the piece's call with the score as its one part (tile_instances does not
    apply: the tiles are the piece's default, by bytes).

    fracs: as render_piece's — voice k starts at onsets[k] + fracs[k] samples; the piece's call with the score as its one part, as
    with pans.

    places (with speakers, decibels_per_metre, sample_delay_per_metre): as render_piece's — mono voices, one channel a speaker; the
    piece's call with the score as its one part, as with pans.

    stereo=True: as render_piece's — voices of one or two channels, two channels out, pans optional and None / NaN for a voice that is
    not placed; the piece's call with the score as its one part, as with pans.

    master: as render_piece's — the mix through a mono circuit, channel by channel, on the device; the piece's call with the score as
    its one part, as with pans.

    tracks, track_of, faders, track_sends: as render_piece's — some of the voices through a circuit of their own before they reach
    the mix; the piece's call with the score as its one part, as with pans.

    stems=True: as render_piece's — the direct mix, every track and every bus return beside the mix, as a Stems; the piece's call with
    the score as its one part, as with a master.

    meters=True, true_peak=True: as render_piece's — the RMS, the loudness and the true peak of every signal the call delivers; the
    piece's call too.  loudness belongs to render_score_pcm and render_score_wav and is refused here."""
    return _render_score(outlets, onsets, voice_duration, duration, lengths, gains, engine, device, tile_instances,
                         _placing(pans, fracs, places, speakers, decibels_per_metre, sample_delay_per_metre, stereo, master, buses, sends, tracks, track_of, faders, track_sends, stems, meters, true_peak, loudness, -1.0, limiter, limiter_window, limiter_release))


def _render_score(outlets, onsets, voice_duration, duration, lengths, gains, engine, device, tile_instances, placing, pcm=None):
    """render_score (pcm None) and render_score_pcm (pcm = (bit_depth, normalise))"""
    if placing["stereo"] or placing["stems"] or placing["meters"] or placing["true_peak"] or placing["loudness"] is not None or placing["limiter"] or any(placing[k] is not None for k in ("pans", "fracs", "space", "master", "buses", "tracks", "limiter_release")):
        return _render_piece_voices(outlets, onsets, _score_voice_duration(voice_duration), duration, lengths, gains, engine, device, 0, placing, True, pcm)
    if pcm is not None:
        _check_pcm(*pcm)
    uni, n_voice, n_total, onsets, lengths, gains, prog = _score_program(outlets, onsets, voice_duration, duration, lengths, gains, engine, device)
    try:
        return _delivered(pcm, uni.sample_rate, n_total, prog.n_out_channels,
                          lambda format, normalise: prog.render_score(n_voice, n_total, uni.n_instances, onsets, lengths, uni.params, gains, tile_instances, format, normalise))
    finally:
        prog.close()


def render_score_pcm(outlets, onsets, voice_duration=1, duration=1, bit_depth=16, normalise=0, lengths=None, gains=None, engine=runtime.ENGINE_AUTO, device=-1,
                     tile_instances=0, pans=None, fracs=None, places=None, speakers=None, decibels_per_metre=-3, sample_delay_per_metre=None, stereo=False, master=None, buses=None, sends=None, tracks=None, track_of=None, faders=None, track_sends=None, stems=False, meters=False, true_peak=False, loudness=None, true_peak_max=-1.0, limiter=False, limiter_window=0.005, limiter_release=None):
    """render_score, delivering what render_pcm delivers: the piece's frames encoded on the device, and its peak -> PcmData (stems=True: a Stems of them, under one gain)."""
    return _render_score(outlets, onsets, voice_duration, duration, lengths, gains, engine, device, tile_instances,
                         _placing(pans, fracs, places, speakers, decibels_per_metre, sample_delay_per_metre, stereo, master, buses, sends, tracks, track_of, faders, track_sends, stems, meters, true_peak, loudness, true_peak_max, limiter, limiter_window, limiter_release), (bit_depth, normalise))


def render_score_wav(outlets, onsets, voice_duration=1, duration=1, bit_depth=16, normalise=0, lengths=None, gains=None, engine=runtime.ENGINE_AUTO, device=-1,
                     tile_instances=0, pans=None, fracs=None, places=None, speakers=None, decibels_per_metre=-3, sample_delay_per_metre=None, stereo=False, master=None, buses=None, sends=None, tracks=None, track_of=None, faders=None, track_sends=None, stems=False, meters=False, true_peak=False, loudness=None, true_peak_max=-1.0, limiter=False, limiter_window=0.005, limiter_release=None):
    """A complete RIFF/WAVE file (bytes) of the piece: render_score_pcm plus the header (wav.encode_wav); stems=True: a Stems of one file a signal."""
    return _wav(render_score_pcm(outlets, onsets, voice_duration, duration, bit_depth, normalise, lengths, gains, engine, device, tile_instances, pans, fracs, places, speakers,
                                 decibels_per_metre, sample_delay_per_metre, stereo, master, buses, sends, tracks, track_of, faders, track_sends, stems, meters, true_peak, loudness, true_peak_max, limiter, limiter_window, limiter_release), bit_depth)


class PieceParts:
    """A voice list grouped into the parts of a piece (piece_parts): parts[p] = (Unified, n_voice_samples) — the voices of one structure
    and one length in samples, unified in the order they come in the list — and, per voice of the list, part_of[k] and instance_of[k]:
    voice k is instance instance_of[k] of part part_of[k], which is also the next unused instance of that part."""

    def __init__(self, parts, part_of, instance_of, sample_rate):
        self.parts, self.part_of, self.instance_of, self.sample_rate = parts, part_of, instance_of, sample_rate


def structure_key(extraction):
    """What two extractions have in common exactly when descriptor.unify takes them as instances of one program: the descriptor's words
    with the values at the constant sites masked (twin of extract.js structureKey)."""
    words = np.array(extraction.words, dtype=np.float64)
    for (_, vpos, cnt) in extraction.const_sites:
        words[vpos:vpos + cnt] = 0
    return words.tobytes()


def piece_parts(extractions, voice_samples):
    """Group the voices of a piece into parts by structure (structure_key) and by voice_samples[k]; parts are numbered in the order their
    first voice comes in the list.  Needs no device.  -> PieceParts"""
    if len(extractions) == 0:
        raise descriptor.DuspError("dusp-hip: no instances")
    rates = {e.sample_rate for e in extractions}
    if len(rates) != 1:
        raise descriptor.DuspError("dusp-hip: the voices of a piece have one sample rate, not %s" % sorted(rates))
    index, members, part_of, instance_of = {}, [], [], []
    for e, n in zip(extractions, voice_samples):
        key = (int(n), structure_key(e))
        if key not in index:
            index[key] = len(members)
            members.append([])
        p = index[key]
        part_of.append(p)
        instance_of.append(len(members[p]))
        members[p].append(e)
    samples = [n for (n, _) in index]  # (dicts keep insertion order: part p's key is the p-th)
    parts = [(descriptor.unify(m), samples[p]) for p, m in enumerate(members)]
    return PieceParts(parts, np.array(part_of, dtype=np.uint32), np.array(instance_of, dtype=np.int64), rates.pop())


def _placing(pans, fracs, places, speakers, decibels_per_metre, sample_delay_per_metre, stereo, master=None, buses=None, sends=None, tracks=None, track_of=None, faders=None, track_sends=None, stems=False, meters=False, true_peak=False, loudness=None, true_peak_max=-1.0, limiter=False, limiter_window=0.005, limiter_release=None):
    """the placement keywords of a call as one thing: what mix.Placement takes once the voices are counted and their sample rate is
    known.  The Space keywords are one thing too, None without places (the other three alone say nothing).  master: what the mix goes
    through behind the placement (master_program makes it a program once the timeline's channels are known), which travels with it;
    buses, sends: the effect buses beside the mix and the voices' levels into them, which travel with it too.  What sends do not go
    with is refused here, before anything else of the call is looked at.  tracks, track_of, faders, track_sends: the tracks some
    voices go through, which travel with it as well; with tracks the buses are fed by track_sends, whatever the placement, and what
    does not go with tracks is refused here too (mix.check_tracks holds the arrays once the voices are counted).  stems: whether the
    call delivers its stems beside the mix, which travels with it too; what is no bool is refused here, first.  meters: whether
    the call also meters what it delivers, which travels with it as stems does and is refused next to it.  true_peak: whether it also
    takes the true peaks, refused next to meters; loudness, true_peak_max: the target and ceiling of a delivery at a loudness target,
    which travel with it as they are (_render_piece_voices holds them to mix.check_loudness once it knows what the call delivers);
    limiter, limiter_window: whether that delivery is limited first and the limiter's window in seconds, which travel the same way
    (mix.check_limiter, once the sample rate is known) — a limiter that is no bool is refused here, next to true_peak; limiter_release:
    the limiter's release in seconds or None, which travels as limiter_window does (mix.check_limiter_release)"""
    stems, meters, true_peak = mix.check_stems(stems), mix.check_meters(meters), mix.check_true_peak(true_peak)
    if not isinstance(limiter, (bool, np.bool_)):
        raise ValueError(mix.LIMITER_NOT_BOOL)
    if tracks is None:
        mix.check_tracks(0, None, track_of, faders, track_sends)
        if buses is None and sends is not None:
            raise ValueError(mix.SENDS_WITHOUT_BUSES)
    else:
        if not isinstance(tracks, (list, tuple)) or not 1 <= len(tracks) <= mix.TRACK_MAX:
            raise ValueError(mix.TRACKS_COUNT % (len(tracks) if isinstance(tracks, (list, tuple)) else 0))
        if track_of is None:
            raise ValueError(mix.TRACKS_WITHOUT_TRACK_OF)
        if sends is not None:
            raise ValueError(mix.TRACKS_WITH_SENDS)
        if track_sends is not None and buses is None:
            raise ValueError(mix.TRACKS_SENDS_WITHOUT_BUSES)
        if buses is not None and track_sends is None:
            raise ValueError(mix.TRACKS_BUSES_WITHOUT_SENDS)
    if buses is not None:
        if tracks is None:
            if sends is None:
                raise ValueError(mix.BUSES_WITHOUT_SENDS)
            if fracs is not None or places is not None or stereo:
                raise ValueError(mix.SENDS_PLACEMENT)
        if not isinstance(buses, (list, tuple)) or not 1 <= len(buses) <= mix.BUS_MAX:
            raise ValueError(mix.BUS_COUNT % (len(buses) if isinstance(buses, (list, tuple)) else 0))
    return dict(pans=pans, fracs=fracs, space=None if places is None else (places, speakers, decibels_per_metre, sample_delay_per_metre), stereo=stereo, master=master,
                buses=buses, sends=sends, tracks=tracks, track_of=track_of, faders=faders, track_sends=track_sends, stems=stems, meters=meters, true_peak=true_peak, loudness=loudness,
                true_peak_max=true_peak_max, limiter=bool(limiter), limiter_window=limiter_window, limiter_release=limiter_release)


def master_program(master, channels, sample_rate, bus=None):
    """The master of a score or piece -> descriptor.Unified of `channels` instances, one a channel of the timeline; needs no device.
    master: a callable fx(x), called once per channel with a fresh graph.MasterInput and returning the master's outlet, or a list of one
    callable a channel (an echo of another length left and right).  The circuits are extracted and unified: they are isomorphic, what
    differs between them is constants, which become the program's parameter table [n_params][channels].  Refused by string: a master
    that is not callable, a list of the wrong length, a circuit that holds no or several MasterInput, a HostSource or a scheduled
    event, one with more than one output channel, circuits that are not isomorphic.
    bus (None: a master): the circuit is bus number `bus` of the call's `buses=` — what a master is to the mix it is to its send
    timeline, given and checked alike, and refused by the BUS_* strings, which name it."""
    return descriptor.unify(_channel_circuits(master, channels, sample_rate, bus))


def _channel_circuits(master, channels, sample_rate, bus=None, track=None):
    """master_program's circuits, extracted and checked, one a channel, before they are unified; track: the circuit is track number
    `track` of the call's `tracks=`, refused by the TRACK_* strings, which name it."""
    from . import graph

    def refuse(name, *args):
        if track is not None:
            raise descriptor.DuspError(getattr(mix, "TRACK_" + name) % ((track,) + args))
        raise descriptor.DuspError(getattr(mix, "MASTER_" + name) % args if bus is None else getattr(mix, "BUS_" + name) % ((bus,) + args))

    fxs = list(master) if isinstance(master, (list, tuple)) else [master] * channels
    if not fxs or not all(callable(fx) for fx in fxs):
        refuse("NOT_CALLABLE")
    if len(fxs) != channels:
        refuse("COUNT" if bus is None and track is None else "CIRCUITS", len(fxs), channels)
    extractions = []
    for c, fx in enumerate(fxs):
        ex = descriptor.extract(fx(graph.MasterInput()), allow_events=True)
        if ex.circuit.events:
            refuse("EVENTS", c)
        if any(not getattr(src, "isMasterInput", False) for src in ex.sources):
            refuse("HOST_SOURCE", c)
        if len(ex.sources) != 1:
            refuse("ONE_INPUT", c, len(ex.sources))
        if ex.sample_rate != sample_rate:
            refuse("RATE", ex.sample_rate, sample_rate)
        n_out = runtime.descriptor_channels(ex.words)
        if n_out != 1:
            refuse("CHANNELS", c, n_out)
        if c and structure_key(ex) != structure_key(extractions[0]):
            refuse("NOT_ISOMORPHIC", c)
        extractions.append(ex)
    return extractions


def track_programs(tracks, channels, sample_rate):
    """The tracks of a score or piece -> a list of (descriptor.Unified, [track numbers]): the tracks' circuits grouped by structure
    (structure_key) in the order their first track comes, every group ONE program whose instances are (track, channel) — instance
    j * channels + c the circuit of the group's j-th track over channel c — and whose parameter table has one column an instance:
    eight tracks with one EQ are one render, not eight.  tracks: a list of 1 .. 8 entries, each None (a track without a circuit: a
    fader group, in no program) or given as a master is, a callable fx(x) over a fresh graph.MasterInput or a list of one a channel.
    Refused by the TRACK_* strings, which name the track, as a master's circuits are.  Needs no device."""
    index, members = {}, []
    for g, fx in enumerate(tracks):
        if fx is None:
            continue
        extractions = _channel_circuits(fx, channels, sample_rate, track=g)
        key = structure_key(extractions[0])
        if key not in index:
            index[key] = len(members)
            members.append(([], []))
        members[index[key]][0].extend(extractions)
        members[index[key]][1].append(g)
    return [(descriptor.unify(extractions), which) for extractions, which in members]


def _piece(outlets, onsets, voice_durations, duration, lengths, gains, placing, one_part=False):
    """-> PieceParts, samples of timeline, onsets, lengths, gains, the timeline's channels, the voices' mix.Placement — with the call's
    master as place.master, a descriptor.Unified of one instance a channel, or None (all checked: nothing is built yet).  placing: the call's placement keywords (_placing); a space becomes the taps of mix.space_taps at the
    voices' sample rate, and parts whose channels do not fit the placement are refused (Placement.timeline_channels)."""
    placing = dict(placing)
    master = placing.pop("master", None)
    buses, sends = placing.pop("buses", None), placing.pop("sends", None)
    tracks, track_of, faders, track_sends = (placing.pop(k, None) for k in ("tracks", "track_of", "faders", "track_sends"))
    stems, meters = placing.pop("stems", False), placing.pop("meters", False)
    true_peak, loudness, true_peak_max = placing.pop("true_peak", False), placing.pop("loudness", None), placing.pop("true_peak_max", -1.0)
    limiter, limiter_window, limiter_release = placing.pop("limiter", False), placing.pop("limiter_window", 0.005), placing.pop("limiter_release", None)
    mix.Placement.refuse_together(placing["pans"], placing["fracs"], placing["space"], placing["stereo"])
    extractions = [descriptor.extract(o) for o in outlets]
    n = len(extractions)
    if n == 0:
        raise descriptor.DuspError("dusp-hip: no instances")
    rate = extractions[0].sample_rate
    durations = np.asarray(voice_durations, dtype=np.float64)
    if durations.ndim == 0:
        durations = np.full(n, float(durations))
    if durations.shape != (n,):
        raise ValueError("dusp-hip: voice_durations must be one number or have shape (voices=%d,)" % n)
    voice_samples = [_n_samples(float(x), rate) for x in durations]
    if min(voice_samples) == 0:
        raise descriptor.DuspError("dusp-hip: voice_duration must cover at least one sample")
    n_total = _n_samples(duration, rate)
    onsets, lengths, gains = _voice_arrays(onsets, lengths, gains, n, np.array(voice_samples), "voices", "the voice's own samples")
    place = mix.Placement(n, sample_rate=rate, **placing)
    grouped = piece_parts(extractions, voice_samples)
    if one_part and len(grouped.parts) != 1:  # (render_score with pans or fracs)
        raise descriptor.DuspError("dusp-hip: the voices of a score are isomorphic circuits: a piece renders several instruments")
    channels = place.timeline_channels([runtime.descriptor_channels(uni.words) for uni, _ in grouped.parts], grouped.part_of)
    place.master = None if master is None else master_program(master, channels, rate)  # (behind every other check of the call)
    place.buses = place.sends = None  # (... and the buses, each a descriptor.Unified of one instance a channel, with the levels [buses, voices])
    place.stems = stems  # (... whether the call delivers its stems)
    place.meters = meters  # (... and whether it meters what it delivers)
    place.true_peak, place.loudness, place.true_peak_max = true_peak, loudness, true_peak_max  # (... takes its true peaks, and delivers at a loudness target)
    place.limiter, place.limiter_window, place.limiter_release = limiter, limiter_window, limiter_release  # (... limited first, with a release of its own)
    place.tracks = None  # (... and the tracks: (how many, track_of, track_programs' groups, faders, levels [buses, tracks]))
    if tracks is not None:
        track_of, faders, track_sends = mix.check_tracks(n, len(tracks), track_of, faders, track_sends, 0 if buses is None else len(buses), sends)
        place.tracks = (len(tracks), track_of, track_programs(tracks, channels, rate), faders, track_sends)
    if buses is not None:
        place.sends = None if tracks is not None else mix.check_sends(sends, n, len(buses))
        place.buses = [master_program(fx, channels, rate, bus=b) for b, fx in enumerate(buses)]
    return grouped, n_total, onsets, lengths, gains, channels, place


def _render_piece(grouped, n_total, onsets, lengths, gains, place, engine, device, tile_bytes, format=None, normalise=0):
    ctx = context(grouped.sample_rate, device)
    programs = []
    try:
        for uni, _ in grouped.parts:
            programs.append(ctx.build(uni.words, engine))
        parts = [(prog, n_voice, uni.n_instances, uni.params) for prog, (uni, n_voice) in zip(programs, grouped.parts)]
        master = getattr(place, "master", None)
        if master is not None:
            programs.append(ctx.build(master.words, engine))
            master = (programs[-1], master.params)
        buses = getattr(place, "buses", None)
        if buses is not None:
            programs.extend(ctx.build(bus.words, engine) for bus in buses)
            buses = [(prog, bus.params) for prog, bus in zip(programs[-len(buses):], buses)]
        tracks = getattr(place, "tracks", None)
        if tracks is not None:
            n_tracks, track_of, groups, faders, track_sends = tracks
            programs.extend(ctx.build(uni.words, engine) for uni, _ in groups)
            circuits = [(prog, which, uni.params) for prog, (uni, which) in zip(programs[len(programs) - len(groups):], groups)]
            tracks = dict(n_tracks=n_tracks, track_of=track_of, programs=circuits, faders=faders, track_sends=track_sends)
        return ctx.render_score_parts(parts, grouped.part_of, onsets, n_total, lengths, gains, tile_bytes, format, normalise, master=master, buses=buses,
                                      sends=getattr(place, "sends", None), tracks=tracks, stems=getattr(place, "stems", False), **(dict(meters=True) if getattr(place, "meters", False) else {}), **getattr(place, "loud", {}), **place.keywords())
    finally:
        for prog in programs:
            prog.close()


def render_piece(outlets, onsets, voice_durations=1, duration=1, lengths=None, gains=None, engine=runtime.ENGINE_AUTO, device=-1, tile_bytes=0, pans=None, _one_part=False,
                 fracs=None, places=None, speakers=None, decibels_per_metre=-3, sample_delay_per_metre=None, stereo=False, master=None, buses=None, sends=None, tracks=None, track_of=None, faders=None, track_sends=None, stems=False, meters=False, true_peak=False, loudness=None, limiter=False, limiter_window=0.005, limiter_release=None):
    """A piece of several instruments: render_score over voices of ANY circuits, each rendered for its own voice_durations[k] seconds
    (one number: all alike).  The voices are grouped into parts by structure and by samples a voice (piece_parts), every part is ONE
    program, and the device walks the caller's voice list in its own order: bit for bit mix.score_chain_rows over what each program
    renders — what `renderChannelData(Sum.many(Delay(outlet_k, onsets[k], maxDelay)), duration)` computes, however the instruments
    interleave.  Voices of one structure and one duration give render_score's bits.  Voices whose circuits differ in output channels are
    refused before anything is built.  onsets and lengths are in SAMPLES (lengths within the voice's own samples), durations in seconds.

    pans (one finite number a voice, -1 left .. +1 right, not clamped): the voices are MONO circuits and voice k is placed in the stereo
    field where it is added to the timeline — what the reference renders for `Pan(voice_k, pans[k])` in the voice's place (with gains:
    `Pan(Multiply(voice_k, g_k), pans[k])`), bit for bit (mix.score_chain_rows_panned).  The result has two channels.

    fracs (one number a voice, 0 <= f < 1; onsets stay whole numbers): voice k starts at onsets[k] + fracs[k] samples — what the
    reference renders for `Delay(., onsets[k] + fracs[k], maxDelay)`, whose two taps carry the weights 1 - frac and frac (mix.two_tap_terms;
    DESIGN.md 6.11 says where the reference's ring departs from it).  dusp_amd.split_onsets makes both arrays from positions in samples
    written as real numbers.  A voice with a fraction covers one more sample; all fractions zero gives the bits of the call without.

    places (one position a voice, 1 to 3 coordinates in metres), with speakers (default [[-1, 0], [1, 0]]; 1 to 8 of them, the same
    number of coordinates), decibels_per_metre (-3) and sample_delay_per_metre (sample rate / 343): the voices are MONO circuits and
    every speaker — a channel of the result — hears voice k attenuated and delayed by its distance, what the reference's Space patch
    does behind a sound: Gain at decibels_per_metre and MonoDelay at sample_delay_per_metre (mix.space_taps makes the gain and the delay
    per voice and speaker with the reference's roundings, mix.score_chain_rows_placed is the contract; DESIGN.md 6.12 says where the
    reference's own wiring departs from it).  Level AND time differences between the speakers, where pans give level only.  Not
    together with pans or fracs.

    stereo=True: a voice may be a MONO circuit or one of TWO channels (StereoDetune, MultiChannelOsc, Multiply(osc, [a, b])), side by
    side, and the result has two channels.  pans may be left out (nothing is placed) or hold None / NaN for a voice that is not placed:
    a mono voice with a pan is the panned voice above, a mono voice without one is heard alike on both channels (the reference's Sum
    reads a mono input for every channel of a wider one), a voice of two channels keeps its channels and takes no pan (the Pan unit's
    inlet is mono).  What the reference renders for Sum.many over such voices behind their Delays, bit for bit
    (mix.score_chain_rows_stereo).  fracs work as above; places are refused.

    master: the mix through a circuit before it is delivered — an EQ, an echo, a comb or all-pass, a clip on the sum — on the device,
    whatever the placement.  A callable fx(x), given a fresh MasterInput once per channel of the timeline and returning a MONO circuit
    over it, or a list of one callable a channel; the circuits are isomorphic and may differ in constants (master_program).  Channel c
    of the result is the render of the master over the timeline's channel c as the chain left it — before `|| 0`, as a unit behind
    Sum.many hears it — from the master's initial state (mix.master_chain; DESIGN.md 6.14 says where that is the reference's
    `fx(Sum.many(...))` bit for bit and where it is not).  The call's engine is the master's too.

    buses, sends: effect sends — some notes, at a level of their own, into an effect such as an echo, and its return beside the dry
    mix.  buses is a list of 1 .. 4 circuits, each given as a master is (a callable fx(x) over a fresh MasterInput, or a list of one
    a channel); sends is float32 [buses, voices] (one bus: [voices] will do), sends[b][k] what voice k gives to bus b.  Bus b hears
    the chain of every voice's dry term — after its gain and its pan — times its level, is rendered over that timeline as a master is
    over the mix, and the buses' outputs are added to the dry mix in order: Sum.many([dry, bus_0(...), bus_1(...), ...]), in front
    of the master where there is one (mix.score_chain_sends, mix.master_chain, mix.bus_return).  A level of 0 is a
    multiplication by 0, not a voice left out.  With plain voices and with pans; fracs, places and stereo are refused with sends.

    tracks, track_of, faders, track_sends: sub-mixes — the drums through one Clip, the pad through one Filter, the bass straight to
    the mix, a fader on each group, the group and not each note sent to the echo.  tracks is a list of 1 .. 8 entries, each given as
    a master is (a callable fx(x) over a fresh MasterInput, or a list of one a channel) or None for a track without a circuit;
    track_of holds one whole number a voice, the track it goes to or -1 for straight to the mix.  Track g hears the chain of ITS
    voices — the call's placement over them alone, in index order, raw — and is rendered over that timeline as a master is over the
    mix; tracks with isomorphic circuits are rendered as ONE program (track_programs).  faders (one finite number a track) scale the
    tracks' outputs, which are added to the direct voices' chain in order; with buses=, track_sends (float32 [buses, tracks]) is what
    each track gives to each bus, and sends= is refused: the buses hear the tracks, not the notes (mix.track_mix).
    Whatever the placement, with or without a master.

    stems=True: the call delivers a Stems — the direct mix (with tracks the voices that go straight to the mix, else the dry mix of
    all voices), every track after its fader and every bus's return, each as the mix is delivered, beside the mix itself, which is
    bit for bit the call's result without stems.  The stems are taken in front of the master; without a master they add up to the mix
    (mix.stems says exactly how).  Every signal comes with its peak, and PCM frames get ONE gain from the largest of
    them, so the files still add up.  One call, one delivery; every signal takes a timeline of device memory.

    meters=True: the call also meters what it delivers, on the device, in front of the PCM gain (mix.meters says exactly what;
    DESIGN.md 6.18): the RMS a channel, the gated integrated loudness in LUFS (ITU-R BS.1770-4) and the momentary loudness of every
    400 ms block, of the mix and — with stems — of every stem.  With stems the Stems gains `.meters`; without, the call returns a
    Metered: `.mix`, what it returns without meters bit for bit, and `.meters`.

    true_peak=True (implies meters): `.meters.true_peak` has the true peak of every channel of every delivered signal — the signal
    oversampled four times (twice from 96 kHz, not at all from 192 kHz) by libebur128's windowed sinc, on the device (mix.true_peak;
    DESIGN.md 6.19) — linear: dBTP is 20 log10.  Everything else is the call with meters=True bit for bit.

    loudness (render_piece_pcm and render_piece_wav; here it is refused): the target in LUFS (-14, -16, -23 ...), with true_peak_max
    the ceiling in dBTP (default -1).  The frames of the mix — and with stems of every stem — are encoded under ONE gain that brings
    the MIX to the target, lowered where the largest true peak of any delivered signal would exceed the ceiling (mix.loudness_gain;
    without limiter=True nothing is limited).  The result gains `.gain` and `.level`; every PcmData.peak stays the signal's sample peak.
    Not together with normalise != 0.

    limiter=True (with loudness; here it is refused) and limiter_window (seconds, default 0.005, at most 4096 samples): a loud
    transient no longer pulls the whole delivery below the target.  Where the largest true peak lies above the ceiling seen from the
    target, every delivered signal is first multiplied by ONE look-ahead gain curve made from the largest oversampled magnitude of
    any of them (mix.limit) — so the stems still add up to the mix — then metered again, and the one gain comes from
    that second measurement: the ceiling is still held by the gain.  The result gains `.limiter` (a Limiter), and where it engaged
    the meters, peaks, gain and level describe the limited signals.

    limiter_release (seconds, with limiter=True; at most 2^22 samples): the limiter's gain then rises by at most 1 / release a second,
    however short the window — a release of 50 to 500 ms instead of the window's 5 (mix.limiter_gain_release).
    `.limiter.release` has it in samples, 0 without one."""
    return _render_piece_voices(outlets, onsets, voice_durations, duration, lengths, gains, engine, device, tile_bytes,
                                _placing(pans, fracs, places, speakers, decibels_per_metre, sample_delay_per_metre, stereo, master, buses, sends, tracks, track_of, faders, track_sends, stems, meters, true_peak, loudness, -1.0, limiter, limiter_window, limiter_release), _one_part)


def _render_piece_voices(outlets, onsets, voice_durations, duration, lengths, gains, engine, device, tile_bytes, placing, one_part, pcm=None):
    """render_piece (pcm None) and render_piece_pcm (pcm = (bit_depth, normalise))"""
    if pcm is not None:
        _check_pcm(*pcm)
    grouped, n_total, onsets, lengths, gains, channels, place = _piece(outlets, onsets, voice_durations, duration, lengths, gains, placing, one_part)
    run = lambda format, normalise: _render_piece(grouped, n_total, onsets, lengths, gains, place, engine, device, tile_bytes, format, normalise)
    names = mix.stem_names(place.tracks[0] if place.tracks is not None else 0, len(place.buses) if place.buses is not None else 0) if place.stems else ["mix"]
    loudness, ceiling = mix.check_loudness(place.loudness, place.true_peak_max, pcm[1] if pcm is not None else 0, pcm is not None)
    window = mix.check_limiter(place.limiter, place.limiter_window, loudness, grouped.sample_rate)
    release = mix.check_limiter_release(place.limiter_release, place.limiter, grouped.sample_rate)
    place.loud = dict(true_peak=True, loudness=loudness, true_peak_max=ceiling) if place.true_peak or loudness is not None else {}
    if window:
        place.loud.update(limiter=True, limiter_window=place.limiter_window)
    if release:
        place.loud.update(limiter_release=place.limiter_release)
    if place.meters or place.loud:  # (the run hands back what it does without meters, and the meters beside it)
        got = _empty_meters(len(names), channels, grouped.sample_rate)
        if place.loud:  # (a timeline of no samples: true peaks 0, gain 1)
            got["true_peak"] = np.zeros((len(names), channels))
        if loudness is not None:
            got["gain"], got["level"] = 1.0, np.float32(1.0)
        if window:  # (... and the limiter has nothing to do)
            got["limiter"] = dict(engaged=False, threshold=0.0, window=window, reduction=1.0, lufs_in=-np.inf, true_peak_in=0.0, release=release)
        render = run

        def run(format, normalise):
            result, metered = render(format, normalise)
            got.update(metered)
            return result

        delivered = (_delivered_stems(pcm, grouped.sample_rate, n_total, channels, names, run) if place.stems else
                     _delivered(pcm, grouped.sample_rate, n_total, channels, run))
        if not place.stems:
            return Metered(delivered, Meters(names, got), got.get("gain"), got.get("level"), Limiter(got["limiter"]) if window else None)
        delivered.meters = Meters(names, got)
        if window:
            delivered.limiter = Limiter(got["limiter"])
        if loudness is not None:  # (the one gain all the frames were encoded under, and the level it came from)
            delivered.gain, delivered.level = got["gain"], got["level"]
        return delivered
    if place.stems:
        return _delivered_stems(pcm, grouped.sample_rate, n_total, channels, names, run)
    return _delivered(pcm, grouped.sample_rate, n_total, channels,
                      lambda format, normalise: _render_piece(grouped, n_total, onsets, lengths, gains, place, engine, device, tile_bytes, format, normalise))


def render_piece_pcm(outlets, onsets, voice_durations=1, duration=1, bit_depth=16, normalise=0, lengths=None, gains=None, engine=runtime.ENGINE_AUTO, device=-1,
                     tile_bytes=0, pans=None, _one_part=False, fracs=None, places=None, speakers=None, decibels_per_metre=-3, sample_delay_per_metre=None, stereo=False, master=None, buses=None, sends=None, tracks=None, track_of=None, faders=None, track_sends=None, stems=False, meters=False, true_peak=False, loudness=None, true_peak_max=-1.0, limiter=False, limiter_window=0.005, limiter_release=None):
    """render_piece, delivering what render_pcm delivers: the piece's frames encoded on the device, and its peak -> PcmData (stems=True: a Stems of them, under one gain)."""
    return _render_piece_voices(outlets, onsets, voice_durations, duration, lengths, gains, engine, device, tile_bytes,
                                _placing(pans, fracs, places, speakers, decibels_per_metre, sample_delay_per_metre, stereo, master, buses, sends, tracks, track_of, faders, track_sends, stems, meters, true_peak, loudness, true_peak_max, limiter, limiter_window, limiter_release), _one_part, (bit_depth, normalise))


def render_piece_wav(outlets, onsets, voice_durations=1, duration=1, bit_depth=16, normalise=0, lengths=None, gains=None, engine=runtime.ENGINE_AUTO, device=-1,
                     tile_bytes=0, pans=None, fracs=None, places=None, speakers=None, decibels_per_metre=-3, sample_delay_per_metre=None, stereo=False, master=None, buses=None, sends=None, tracks=None, track_of=None, faders=None, track_sends=None, stems=False, meters=False, true_peak=False, loudness=None, true_peak_max=-1.0, limiter=False, limiter_window=0.005, limiter_release=None):
    """A complete RIFF/WAVE file (bytes) of the piece: render_piece_pcm plus the header (wav.encode_wav); stems=True: a Stems of one file a signal."""
    return _wav(render_piece_pcm(outlets, onsets, voice_durations, duration, bit_depth, normalise, lengths, gains, engine, device, tile_bytes, pans, fracs=fracs, places=places,
                                 speakers=speakers, decibels_per_metre=decibels_per_metre, sample_delay_per_metre=sample_delay_per_metre, stereo=stereo, master=master, buses=buses, sends=sends, tracks=tracks, track_of=track_of, faders=faders, track_sends=track_sends, stems=stems, meters=meters, true_peak=true_peak, loudness=loudness, true_peak_max=true_peak_max, limiter=limiter, limiter_window=limiter_window, limiter_release=limiter_release), bit_depth)


class PcmData:
    """Encoded frames of one render: `data` int16 [samples, channels] (bitDepth 16), uint8 [samples, channels, 3] (24) or float32
    [samples, channels] (32); `peak` is the render's max |x| before the gain.  wav.encode_wav(data, sampleRate, bitDepth) makes a file of it."""

    def __init__(self, data, bit_depth, sample_rate, peak):
        self.data, self.bitDepth, self.sampleRate, self.peak = data, bit_depth, sample_rate, np.float32(peak)
        self.numberOfChannels = data.shape[1]


_PCM_FORMAT = {16: "s16", 24: "s24", 32: "f32"}


def render_pcm(outlet, duration=1, bit_depth=16, normalise=0, engine=runtime.ENGINE_AUTO, device=-1):
    """renderChannelData, delivering peak-normalised 16- / 24-bit (or f32) frames -> PcmData.  normalise: 0 none, 1 shrink only a render
    that would clip, 2 to full scale; one gain for all channels (include/dusp_hip.h "Device-side PCM delivery" is the sample contract).

    An event-free circuit is encoded on the device (Program.render_pcm): peak, gain, quantisation and interleave run there and 2 or 3
    bytes per sample are downloaded.  A circuit with scheduled events is rendered in segments that arrive as f32 on the host
    (renderChannelData); those are encoded here by the same contract (wav.encode_frames), the peak taken over the whole render.  The
    bytes are the same either way.  Like renderChannelData this consumes the circuit."""
    _check_pcm(bit_depth, normalise)
    first = _no_master_input(descriptor.extract(outlet, allow_events=True))
    n = _n_samples(duration, first.sample_rate)
    if n > 0 and not first.circuit.events:
        prog = context(first.sample_rate, device).build(first.words, engine)
        try:
            data, peaks = prog.render_pcm(n, 1, format=_PCM_FORMAT[bit_depth], normalise=normalise, inputs=_host_inputs(first.sources, 0, n))
            write_back(prog, first.circuit, first.chunk_size, n)
        finally:
            prog.close()
        return PcmData(data[0], bit_depth, first.sample_rate, peaks[0])
    channels = _render_extracted(outlet, first, duration, np.float32, engine, device)
    planar = np.stack([np.asarray(c, dtype=np.float32) for c in channels]) if n > 0 else np.zeros((1, 0), dtype=np.float32)
    data, peak = wav.encode_frames(planar, bit_depth, normalise)
    return PcmData(data, bit_depth, first.sample_rate, peak)


def render_wav(outlet, duration=1, bit_depth=16, normalise=0, engine=runtime.ENGINE_AUTO, device=-1):
    """A complete RIFF/WAVE file (bytes) of the render: render_pcm plus the header (wav.encode_wav)."""
    return _wav(render_pcm(outlet, duration, bit_depth, normalise, engine, device), bit_depth)
