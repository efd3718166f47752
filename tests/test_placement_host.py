"""mix.Placement without a device: the keywords of a call as one checked record — its kind, its arrays, the two orders of refusal, the
combination refusals, the timeline's channels for the parts, and the chain it names, bit for bit the chain functions themselves."""
import numpy as np
import pytest

from dusp_amd import DuspError, mix
from dusp_amd.mix import Placement

TAPS = ([[0.0, 1.5], [2.25, 0.0], [3.0, 4.5]], [[1.0, 0.5], [0.25, 1.0], [0.5, 0.5]])
SPACE = ([[0.0, 1.0], [0.5, 2.0], [-1.0, 0.25]], None, -3, None)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_the_kind_the_arrays_and_the_keywords_of_every_placement():
    plain = Placement(3)
    assert plain.kind == "rows" and plain.pans is plain.comp is plain.fracs is plain.taps is None
    assert plain.keywords() == dict(pans=None, fracs=None, taps=None, stereo=False) and plain.channels(5) == 5
    frac = Placement(3, fracs=[0, 0.5, 0.25])
    assert frac.kind == "rows" and frac.fracs.dtype == np.float64 and frac.fracs.tolist() == [0, 0.5, 0.25] and frac.channels(2) == 2
    pan = Placement(3, pans=[-1, 0.3, 1.5], fracs=[0, 0.5, 0])
    assert pan.kind == "pan" and pan.pans.dtype == np.float32 and np.array_equal(pan.comp, mix.pan_comp(pan.pans)) and pan.channels(1) == 2
    assert Placement(3, pans=[0, 0, 0], comp=[1.0, 2.0, 3.0]).comp.tolist() == [1.0, 2.0, 3.0]
    space = Placement(3, taps=TAPS)
    assert space.kind == "space" and space.taps[0].shape == (3, 2) and space.channels(1) == 2 and space.keywords()["taps"] is space.taps
    stereo = Placement(3, pans=[0.5, None, float("nan")], stereo=True)
    assert stereo.kind == "stereo" and stereo.keywords()["stereo"] is True and stereo.channels(1) == 2
    assert stereo.pans[0] == 0.5 and np.isnan(stereo.pans[1:]).all() and stereo.comp[1] == 1.0
    assert np.isnan(Placement(3, stereo=True).pans).all()


def test_a_space_is_the_taps_of_space_taps_at_the_sample_rate():
    place = Placement(3, space=SPACE, sample_rate=48000)
    delays, gains = mix.space_taps(SPACE[0], sample_rate=48000)
    assert place.kind == "space" and np.array_equal(place.taps[0], delays) and np.array_equal(place.taps[1], gains) and place.channels(1) == 2


def test_what_does_not_go_together_is_refused_first():
    for make in (lambda **kw: Placement(3, **kw), lambda pans=None, fracs=None, taps=None, stereo=False: Placement.refuse_together(pans, fracs, taps, stereo)):
        with pytest.raises(ValueError) as e:
            make(taps=TAPS, stereo=True, pans=[0], fracs=[7])
        assert str(e.value) == mix.STEREO_NO_PLACES
        for kw in (dict(pans=[0]), dict(fracs=[7]), dict(pans=[0], fracs=[7])):
            with pytest.raises(ValueError) as e:
                make(taps=TAPS, **kw)
            assert str(e.value) == mix.SPACE_ALONE
    with pytest.raises(ValueError) as e:
        Placement(3, space=SPACE, stereo=True, sample_rate=48000)
    assert str(e.value) == mix.STEREO_NO_PLACES


def test_pans_are_refused_before_fracs_unless_the_fractions_come_first():
    with pytest.raises(ValueError) as e:
        Placement(3, pans=[0], fracs=[2, 2, 2])
    assert str(e.value) == "dusp-hip: pans must have shape (voices=3,)"
    with pytest.raises(ValueError) as e:
        Placement(3, pans=[0], fracs=[2, 2, 2], fracs_first=True)
    assert str(e.value) == "dusp-hip: the fraction of voice 0 is outside [0, 1)"
    with pytest.raises(ValueError) as e:
        Placement(3, pans=[0, None, float("inf")], fracs=[2, 2, 2], stereo=True)
    assert str(e.value) == "dusp-hip: the pan of voice 2 is not finite"
    with pytest.raises(ValueError) as e:
        Placement(3, taps=([[0.0]] * 3, [[1.0]] * 2))
    assert str(e.value) == "dusp-hip: the taps' delays and gains must both have shape (voices=3, speakers)"


def test_the_timelines_channels_for_the_parts_and_the_parts_that_do_not_fit():
    assert Placement(3).timeline_channels([2, 2], [0, 1, 0]) == 2
    assert Placement(3, pans=[0, 0, 0]).timeline_channels([1, 1], [0, 1, 0]) == 2
    assert Placement(3, taps=TAPS).timeline_channels([1], [0, 0, 0]) == 2
    assert Placement(3, pans=[0.5, None, None], stereo=True).timeline_channels([1, 2], [0, 1, 0]) == 2
    for place, channels, refusal in (
            (Placement(3), [2, 1], "dusp-hip: the voices of a piece must have one number of output channels: part 1 has 1, part 0 has 2"),
            (Placement(3, pans=[0, 0, 0]), [1, 2], "dusp-hip: a panned voice is mono: part 1 has 2 output channels"),
            (Placement(3, taps=TAPS), [1, 2], "dusp-hip: a placed voice is mono: part 1 has 2 output channels")):
        with pytest.raises(DuspError) as e:
            place.timeline_channels(channels, [0, 1, 0])
        assert str(e.value) == refusal
    with pytest.raises(ValueError) as e:
        Placement(3, pans=[0.5, 0.5, None], stereo=True).timeline_channels([1, 2], [0, 1, 0])
    assert str(e.value) == "dusp-hip: a two-channel voice is not panned: the pan of voice 1 must be NaN (not placed)"


def test_the_chain_a_placement_names_is_that_chain_bit_for_bit():
    rng = np.random.default_rng(7)
    mono = [rng.standard_normal((1, n)).astype(np.float32) for n in (9, 5, 12)]
    wide = [rng.standard_normal((2, n)).astype(np.float32) for n in (9, 5, 12)]
    mixed = [mono[0], wide[1], mono[2]]
    onsets, lengths, gains, fracs, nt = [-2, 3, 6], [9, 4, 12], [0.5, -1.25, 2.0], [0.5, 0, 0.125], 17
    init = rng.standard_normal((2, nt)).astype(np.float32)
    pans, comp = [-1, 0.3, 1.5], [1.0, 1.1, 0.9]
    same = lambda got, want: np.array_equal(bits(got), bits(want))
    place = Placement(3, fracs=fracs)
    assert place.chain is mix.score_chain_rows and Placement(3).chain is mix.score_chain_rows
    assert same(place.chain(wide, onsets, nt, lengths, gains, init, True, place.fracs), mix.score_chain_rows(wide, onsets, nt, lengths, gains, init, True, fracs))
    place = Placement(3, pans, comp, fracs)
    assert place.chain is mix.score_chain_rows_panned
    assert same(place.chain(mono, onsets, place.pans, nt, lengths, gains, init, False, place.comp, place.fracs),
                mix.score_chain_rows_panned(mono, onsets, pans, nt, lengths, gains, init, False, comp, fracs))
    place = Placement(3, pans)
    assert same(place.chain(mono, onsets, place.pans, nt, comp=place.comp), mix.score_chain_rows_panned(mono, onsets, pans, nt))
    place = Placement(3, taps=TAPS)
    assert place.chain is mix.score_chain_rows_placed
    assert same(place.chain(mono, onsets, *place.taps, nt, lengths, gains, init, True), mix.score_chain_rows_placed(mono, onsets, TAPS[0], TAPS[1], nt, lengths, gains, init, True))
    place = Placement(3, [0.5, None, None], fracs=fracs, stereo=True)
    assert place.chain is mix.score_chain_rows_stereo
    assert same(place.chain(mixed, onsets, place.pans, nt, lengths, gains, init, False, place.comp, place.fracs),
                mix.score_chain_rows_stereo(mixed, onsets, [0.5, None, None], nt, lengths, gains, init, False, None, fracs))
