"""Which refusal a call of the piece entry with TWO faults gets (dusp_render_host_score_piece_meters, the entry that takes everything a
piece can have): 'which refusal a call with several faults gets is behaviour'.  The two faults of every case are looked at by different
stages of the entry — the placement record, the voices' arrays, the taps, the parts, the master, the buses, the tracks, the stems, the
meters, the timeline, the values, the chain's instances, the kinds, the tiles, the plans — and the expected message is the one the
library gave before the entry was cut into those stages.  Nothing renders before a refusal: h_out is as it was."""
import ctypes

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
from dusp_amd import descriptor, mix, runtime

pytestmark = pytest.mark.gpu

RATE = sv.SAMPLE_RATE
NVS = 256  # samples a voice is rendered for
NT = 600   # samples of timeline
WHO = "dusp_render_host_score_piece_meters: "


def test_a_call_with_two_faults_gets_the_refusal_of_the_earlier_check():
    d.configure(RATE)
    L = runtime.load()
    ctx, other = runtime.Context(-1, RATE), runtime.Context(-1, RATE)
    two = descriptor.unify([descriptor.extract(sv.voice(k)) for k in range(2)])
    echo = mc.unified_master([mc.echo_of(300.25)], 1)
    P = dict(part=ctx.build(two.words), part_elsewhere=other.build(two.words), good=ctx.build(echo.words), good2=ctx.build(echo.words), elsewhere=other.build(echo.words))
    out = np.full((8, NT), 7, dtype=np.float32)
    peaks = np.zeros(8, dtype=np.float32)
    rms, lufs = np.zeros((8, 2)), np.zeros(8)
    n_blocks = mix.meter_blocks(NT, RATE)
    keep = []

    def held(a, dtype):
        keep.append(np.ascontiguousarray(a, dtype=dtype))
        return keep[-1].ctypes.data

    def call(n_voices=2, part_of=(0, 0), onsets=(0, 40), lengths=None, part_instances=2, second_part=None, place=None, master=None, buses=None, sends=None, tracks=None,
             stems=None, meters=None, n_total=NT, fmt=0, h_out=True):
        parts = [runtime.ScorePart(P["part"]._h, part_instances, NVS, two.params.ctypes.data)]
        if second_part is not None:
            parts.append(runtime.ScorePart(second_part._h, 1, NVS, two.params.ctypes.data))
        table = (runtime.ScorePart * len(parts))(*parts)
        how = None
        if place is not None:
            kind, fracs, pans, speakers, delays = place
            how = runtime.ScorePlacement(runtime.PLACE_KINDS[kind], None if fracs is None else held(fracs, np.float64), None if pans is None else held(pans, np.float32), None, speakers,
                                         None if delays is None else held(delays, np.float64), None if delays is None else held(np.ones_like(delays), np.float64))
        through = runtime.ScoreMaster(master, None) if master is not None else None
        into = None
        if buses is not None:
            bus_table = (runtime.ScoreMaster * max(len(buses), 1))(*[runtime.ScoreMaster(b._h, None) for b in buses])
            into = runtime.ScoreBuses(len(buses), ctypes.addressof(bus_table), None if sends is None else held(sends, np.float32))
        routed = None
        if tracks is not None:
            circuits = tracks.get("programs", [])
            table_t = (runtime.ScoreTrackProgram * max(len(circuits), 1))(*[runtime.ScoreTrackProgram(prog._h, len(which), held(which, np.uint32), None) for prog, which in circuits])
            routed = runtime.ScoreTracks(tracks["n_tracks"], held(tracks["track_of"], np.int32), len(circuits), ctypes.addressof(table_t),
                                         None if tracks.get("faders") is None else held(tracks["faders"], np.float32),
                                         None if tracks.get("track_sends") is None else held(tracks["track_sends"], np.float32))
        asked = runtime.ScoreStems(stems) if stems is not None else None
        want = None
        if meters is not None:
            want = runtime.ScoreMeters(meters.get("n_signals", 1), meters.get("n_blocks", n_blocks), None if meters.get("null_rms") else rms.ctypes.data, lufs.ctypes.data, None)
        at = lambda record: ctypes.addressof(record) if record is not None else None
        return L.dusp_render_host_score_piece_meters(table, len(parts), n_voices, held(part_of, np.uint32), None if onsets is None else held(onsets, np.int64),
                                                     None if lengths is None else held(lengths, np.int64), None, at(how), at(routed), at(into), at(through), at(asked), at(want),
                                                     n_total, 0, fmt, 0, out.ctypes.data if h_out else None, peaks.ctypes.data)

    nan = float("nan")
    too_long = (NVS + 1, 10)  # (the plans' refusal: the last stage that refuses)
    beside = [0.5, 1.5]       # (a fraction outside [0, 1): the values')
    try:
        for name, kw, needle, status in [
            ("a tap's delay, a part on another context",
             dict(place=("space", None, None, 2, np.array([[0.0, 1.0], [-1.0, 2.0], [0.0, 0.0]])), second_part=P["part_elsewhere"], n_voices=3, part_of=(0, 0, 1), onsets=(0, 40, 80)),
             "the delay of voice 1 at speaker 0 is outside [0, 2^24] samples", -1),
            ("a bus that is the master, a fader that is not finite",
             dict(tracks=dict(n_tracks=2, track_of=(0, -1), faders=[1, nan], track_sends=np.ones((1, 2))), buses=[P["good"]], master=P["good"]._h),
             "bus 0 is also the master", -1),
            ("the stems' n_signals, a fraction outside [0, 1)", dict(place=("rows", beside, None, 0, None), stems=5), "the stems' n_signals is 5, the call delivers 2", -1),
            ("the meters' n_blocks, a voice of a missing part", dict(meters=dict(n_blocks=n_blocks + 3), part_of=(0, 3)), "the meters' n_blocks is %d" % (n_blocks + 3), -1),
            ("a track with two circuits, a length out of range",
             dict(tracks=dict(n_tracks=2, track_of=(0, -1), programs=[(P["good"], [0]), (P["good2"], [1, 0])]), lengths=too_long),
             "track program 1 lists track 0, which has a circuit already", -1),
            ("a fraction outside [0, 1), a voice of a missing part", dict(place=("rows", beside, None, 0, None), part_of=(0, 3)), "the fraction of voice 1 is outside [0, 1)", -1),
            ("a voice of a missing part, a length out of range", dict(part_of=(0, 3), lengths=too_long), "voice 1 names part 3 of 1", -1),
            ("a master on another context, no buses", dict(master=P["elsewhere"]._h, buses=[], sends=np.ones((1, 2))), "the master was built on another context", -1),
            ("a send level that is not finite, the meters' h_rms NULL",
             dict(buses=[P["good"]], sends=[[nan, 1]], meters=dict(null_rms=True)), "the send level of voice 0 into bus 0 is not finite", -1),
            ("no voices, a master without a program", dict(n_voices=0, master=0), "need 1..2^24 voices", -1),
            ("pans that are NULL, onsets that are NULL", dict(place=("pan", None, None, 0, None), onsets=None), "h_pans is NULL", -1),
            ("stems without h_out, the meters' n_signals", dict(stems=2, h_out=False, meters=dict(n_signals=7)), "h_out is NULL: a call with stems delivers its 2 signals there", -1),
            ("a master over too long a timeline, a pan that is not finite",
             dict(place=("pan", None, [float("inf"), 0], 0, None), master=P["good"]._h, n_total=(1 << 31) + 1), "the master renders channels x timeline samples, which must not exceed 2^31", -1),
            ("a part's instances, a length out of range", dict(part_instances=3, lengths=too_long), "h_part_of names part 0 2 times, the part has 3 instances", -1),
            ("a stereo voice's pan, a part's instances", dict(place=("stereo", None, [float("inf"), nan], 0, None), part_instances=3), "the pan of voice 0 is not finite", -1),
            ("the format, a length out of range", dict(fmt=9, lengths=too_long), "format must be 0 (planar f32), DUSP_PCM_S16 (1), DUSP_PCM_S24 (2) or DUSP_PCM_F32 (3)", -1),
            ("no timeline, a fraction outside [0, 1)", dict(place=("rows", beside, None, 0, None), n_total=0), "the timeline must have 1..2^31 samples", -1),
        ]:
            rc = call(**kw)
            message = L.dusp_last_error(ctx._h).decode()
            print("%-60s %d %s" % (name, rc, message))
            assert rc == status and message.startswith(WHO) and needle in message, (name, rc, message)
            assert (out == 7).all(), "a refused call wrote to h_out: " + name
        # the calls above are refused for what they bend alone: unbent, the call renders
        assert call(meters=dict()) == 0, L.dusp_last_error(ctx._h).decode()
        assert not (out[0] == 7).any() and (out[1:] == 7).all() and rms[0, 0] > 0
    finally:
        for prog in P.values():
            prog.close()
        ctx.close()
        other.close()
