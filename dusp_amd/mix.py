"""The mix of a batch of voices in `Sum.many`'s chain order: the contract of dusp_mix_device, in numpy (needs no GPU).

The reference's `Sum.many(voices)` is a left-deep chain ((v0 + v1) + v2) + ... of Sum units, each of which stores its result in
a Float32Array (src/components/Sum.js:18-29,33-44): one f32 rounding per add, in index order.  A gain per voice is a Multiply in
front of the chain: one f32 rounding per product (Multiply.js:23-34)."""
import numpy as np

from .descriptor import DuspError


def mix_chain(planar, gains=None, init=None, raw=False):
    """planar float32 [instances, channels, samples] -> float32 [channels, samples].

        acc = init if given else term(0);  acc = f32(acc + term(i)) for the remaining instances in index order
        term(i) = f32(planar[i] * gains[i]) if gains is given else planar[i]

    Without `init` the chain starts from the first voice itself, not from 0 + v0.  raw: the sums as they stand (a partial sum to be
    continued through `init`: NaN and -0 kept); otherwise NaN and -0 become +0, the `x || 0` of renderChannelData.js:44."""
    planar = np.asarray(planar, dtype=np.float32)
    if planar.ndim != 3 or planar.shape[0] < 1:
        raise ValueError("dusp-hip: planar must have shape (instances >= 1, channels, samples)")
    gains = _gains_table(gains, planar.shape[0], "instances")
    if init is not None:
        init = np.asarray(init, dtype=np.float32)
        if init.shape != planar.shape[1:]:
            raise ValueError("dusp-hip: init must have shape (channels=%d, samples=%d)" % planar.shape[1:])

    def term(i):
        return planar[i] if gains is None else planar[i] * gains[i]  # float32 * float32 scalar: one f32 rounding

    with np.errstate(all="ignore"):
        acc = init.copy() if init is not None else np.array(term(0), dtype=np.float32)
        for i in range(0 if init is not None else 1, planar.shape[0]):
            acc = acc + term(i)  # float32 + float32: one f32 rounding
        return _chain_end(acc, raw)


def score_chain(planar, onsets, n_total, lengths=None, gains=None, init=None, raw=False):
    """planar float32 [instances, channels, voice samples], onsets int64 [instances] -> float32 [channels, n_total]: the contract of
    dusp_score_device.  Voice k lies on the timeline at samples onset_k .. onset_k + len_k - 1 (any sign; lengths None: the whole row);
    for every channel c and timeline sample t

        acc = init[c][t] if init is given else +0
        for k in index order:  s = t - onset_k;  if 0 <= s < len_k:  acc = f32(acc + term_k),
                               term_k = f32(planar[k][c][s] * gains[k]) if gains is given else planar[k][c][s]
        out[c][t] = acc if raw else (acc || 0)

    A voice takes no part in a sample outside its span: nothing is added there, not even a zero, so a raw partial sum continued through
    `init` is the same chain wherever it is cut (tiles of voices, windows of the timeline with their onsets shifted).  Unlike mix_chain
    the chain starts from +0, not from the first voice itself: a lone -0 sample leaves a raw chain as +0.  It is what the reference's
    `Sum.many(Delay(voice_k, onset_k, maxDelay))` renders (Delay.js:27-38: an integer delay is the input shifted behind zeros)."""
    planar = np.asarray(planar, dtype=np.float32)
    if planar.ndim != 3:
        raise ValueError("dusp-hip: planar must have shape (instances, channels, samples)")
    n_inst, n_ch, n_voice = planar.shape
    n_total = _timeline(n_total)
    onsets = _whole(onsets, n_inst, "onsets", "instances")
    if lengths is None:
        lengths = np.full(n_inst, n_voice, dtype=np.int64)
    else:
        lengths = _whole(lengths, n_inst, "lengths", "instances")
        if np.any(lengths < 0) or np.any(lengths > n_voice):
            raise ValueError("dusp-hip: lengths must lie in 0 .. samples=%d" % n_voice)
    return _chain(list(planar), n_ch, n_total, onsets, lengths, gains, None, init, raw, noun="instances")


def _timeline(n_total):
    if int(n_total) != n_total or n_total < 0:
        raise ValueError("dusp-hip: n_total must be a whole number of samples, not negative")
    return int(n_total)


def _whole(values, n, name, noun="voices", refusal="dusp-hip: %s are whole numbers of samples"):
    """onsets / lengths of n voices -> int64 [n] (contiguous): whole numbers of samples, refused otherwise in the caller's words (the
    noun of the shape, and the sentence for what is no whole number; dusp_amd/runtime.py _whole_samples has its own)"""
    a = np.asarray(values)
    if a.shape != (n,):
        raise ValueError("dusp-hip: %s must have shape (%s=%d,)" % (name, noun, n))
    if a.dtype.kind not in "iu":
        if a.dtype.kind != "f" or not np.all(np.isfinite(a)) or np.any(a != np.floor(a)) or np.any(np.abs(a) >= 2.0 ** 63):
            raise ValueError(refusal % name)
    return a.astype(np.int64)


def _row_lengths(rows, lengths):
    """lengths of voices that each lie in a row of their own -> int64 [voices]: None for the whole rows, else checked against them"""
    samples = np.array([r.shape[1] for r in rows], dtype=np.int64)
    if lengths is None:
        return samples
    lengths = _whole(lengths, len(rows), "lengths")
    if np.any(lengths < 0) or np.any(lengths > samples):
        k = int(np.argmax((lengths < 0) | (lengths > samples)))
        raise ValueError("dusp-hip: the length of voice %d is %d: lengths must lie in 0 .. the row's samples (%d)" % (k, int(lengths[k]), int(samples[k])))
    return lengths


def _gains_table(gains, n, noun="voices"):
    """gains -> contiguous float32 [n], checked, or None; noun: what the caller counts (n_instances, instances, voices)"""
    if gains is not None:
        gains = np.ascontiguousarray(gains, dtype=np.float32)
        if gains.shape != (n,):
            raise ValueError("dusp-hip: gains must have shape (%s=%d,)" % (noun, n))
    return gains


def _chain_start(init, n_ch, n_total):
    """what a chain starts from -> float32 [n_ch, n_total]: a copy of init, checked, or +0"""
    if init is None:
        return np.zeros((n_ch, n_total), dtype=np.float32)
    init = np.asarray(init, dtype=np.float32)
    if init.shape != (n_ch, n_total):
        raise ValueError("dusp-hip: init must have shape (channels=%d, n_total=%d)" % (n_ch, n_total))
    return init.copy()


def _chain_end(acc, raw):
    """what a chain hands back: the sums as they stand (raw), or NaN and -0 as +0 (`acc || 0`)"""
    assert acc.dtype == np.float32
    with np.errstate(all="ignore"):
        return acc if raw else np.where(np.isnan(acc) | (acc == 0), np.float32(0), acc)


def _chain(rows, n_ch, n_total, onsets, lengths, gains, fracs, init, raw, noun="voices", place=None, sends=None):
    """The one chain behind score_chain, score_chain_rows and score_chain_rows_panned.  rows: a list of float32 [channels, samples_k];
    onsets, lengths: int64 [voices], checked by the caller; gains, fracs and init are checked here, in that order (they are refused in
    the same words by all three, but for the noun of the gains' shape).  place(k, x): what becomes of voice k's samples after the gain
    before they are added, float32 [channels, len] -> float32 [n_ch, len] (None: x itself).
    sends (None: the chain as it always was, operation for operation): float32 [B, voices], checked by the caller (check_sends), without
    fracs — the term every add of the chain adds is also multiplied by sends[b][k], a plain f32 product, and added to bus b's send
    timeline by a plain f32 add, for every bus and every voice (score_chain_sends).  Then -> (sums, send timelines [B, n_ch, n_total])."""
    gains = _gains_table(gains, len(rows), noun)
    if fracs is not None:
        fracs = check_fracs(fracs, len(rows))
    acc = _chain_start(init, n_ch, n_total)
    send = None if sends is None else np.zeros((len(sends), n_ch, n_total), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k, row in enumerate(rows):
            onset, length = int(onsets[k]), int(lengths[k])
            frac = fracs[k] if fracs is not None and length > 0 else 0  # (a voice of length 0 takes no part)
            span = length + 1 if frac != 0 else length  # with a fraction the span is one sample longer: the last sample's ceil tap
            t0, t1 = max(onset, 0), min(onset + span, n_total)  # (Python integers: no overflow)
            if t1 <= t0:
                continue
            x = row[:, :length] if frac != 0 else row[:, t0 - onset:t1 - onset]
            if gains is not None:
                x = x * gains[k]  # float32 * float32 scalar: one f32 rounding
            if place is not None:
                x = place(k, x)
            term = two_tap_terms(x, frac)[:, t0 - onset:t1 - onset] if frac != 0 else x
            # float32 + float32: one f32 rounding.  A placed voice without a fraction is added channel by channel, as it always was: the
            # sums are the same numbers, but where BOTH operands are NaN the arrays' layout decides which NaN's bits numpy keeps.
            if place is None or frac != 0:
                acc[:, t0:t1] = acc[:, t0:t1] + term
            else:
                for c in range(n_ch):
                    acc[c, t0:t1] = acc[c, t0:t1] + term[c]
            if send is not None:  # (term: float32 [n_ch, t1 - t0], the very values added above)
                for b in range(len(sends)):
                    for c in range(n_ch):
                        send[b, c, t0:t1] = send[b, c, t0:t1] + term[c] * sends[b, k]  # one f32 product, one f32 add
    return _chain_end(acc, raw) if send is None else (_chain_end(acc, raw), send)


def check_fracs(fracs, n):
    """fracs of n voices -> contiguous float64 [n]: checked — one finite fraction of a sample a voice, 0 <= f < 1 — by the strings the C
    calls use (dusp_score_rows_frac_device).  Needs no device."""
    with np.errstate(all="ignore"):
        fracs = np.ascontiguousarray(fracs, dtype=np.float64)
    if fracs.shape != (n,):
        raise ValueError("dusp-hip: fracs must have shape (voices=%d,)" % n)
    if not np.all(np.isfinite(fracs)):
        raise ValueError("dusp-hip: the fraction of voice %d is not finite" % int(np.argmax(~np.isfinite(fracs))))
    if np.any((fracs < 0) | (fracs >= 1)):
        raise ValueError("dusp-hip: the fraction of voice %d is outside [0, 1)" % int(np.argmax((fracs < 0) | (fracs >= 1))))
    return fracs


def split_onsets(positions):
    """Positions on the timeline in samples, real numbers of any sign -> (int64 onsets, float64 fracs) by floor: position = onset + frac
    with 0 <= frac < 1, what the `onsets` and `fracs` of a score or piece take.  position - floor(position) is exact in float64 except
    for a negative position so close to a whole number that the difference rounds to 1.0 (-1e-300, say): that position IS the whole
    number above it as far as a double can tell, and becomes (floor + 1, 0.0).  A position of magnitude 2^52 and beyond is a whole
    number already.  Positions are finite and within int64."""
    with np.errstate(all="ignore"):
        p = np.asarray(positions, dtype=np.float64)
    if not np.all(np.isfinite(p)) or np.any(p >= 2.0 ** 63) or np.any(p < -2.0 ** 63):
        raise ValueError("dusp-hip: positions are finite numbers of samples within int64")
    whole = np.floor(p)
    frac = p - whole
    up = frac >= 1.0
    return (whole + up).astype(np.int64), np.where(up, 0.0, frac)


def two_tap_terms(x, frac):
    """What a voice with a fraction adds to the timeline: x float32 [..., len] (len >= 1), the voice's samples after gain (and pan) ->
    float32 [..., len + 1], the terms of the timeline samples onset .. onset + len.  The reference's Delay writes every input sample to
    two neighbouring ring slots with the weights 1 - frac and frac (Delay.js:36-38); the ceil tap of sample s - 1 is alone in its slot
    when the floor tap of sample s is added to it:

        w1 = frac, w0 = 1.0 - frac                       (one f64 subtraction)
        c(s)      = f32(f64(x[s-1]) * w1)                1 <= s <= len
        term(0)   = f32(f64(x[0]) * w0)
        term(s)   = f32(f64(c(s)) + f64(x[s]) * w0)      1 <= s < len     (every f64 operation rounded by itself: no FMA)
        term(len) = c(len)"""
    x = np.asarray(x, dtype=np.float32)
    w1 = np.float64(frac)
    w0 = np.float64(1.0) - w1
    with np.errstate(all="ignore"):
        xd = x.astype(np.float64)
        c = (xd * w1).astype(np.float32)  # c[..., s - 1] is c(s)
        floor_tap = xd * w0
        terms = np.empty(x.shape[:-1] + (x.shape[-1] + 1,), dtype=np.float32)
        terms[..., 0] = floor_tap[..., 0].astype(np.float32)
        terms[..., 1:-1] = (c[..., :-1].astype(np.float64) + floor_tap[..., 1:]).astype(np.float32)
        terms[..., -1] = c[..., -1]
    return terms


def score_chain_rows(rows, onsets, n_total, lengths=None, gains=None, init=None, raw=False, fracs=None):
    """rows: a list of float32 arrays [channels, samples_k] — every voice a row of its own length, all of one channel count — onsets
    int64 [voices] -> float32 [channels, n_total]: the contract of dusp_score_rows_device.  The chain is score_chain's, word for word: it
    starts from `init` or +0, the voices go in index order, voice k takes part only where 0 <= t - onset_k < len_k (lengths None: the
    whole row; else 0 <= len_k <= samples_k), a term is f32(x * g_k) when gains are given, one f32 rounding per add, and `acc || 0`
    unless raw.  Rows of one length give exactly score_chain of their stack; a piece of several instruments, each rendered for its own
    note length, is one such chain over the voices in the caller's order.

    fracs (float64 [voices], 0 <= f < 1; None: today's chain, untouched): voice k starts at onset_k + frac_k samples.  A voice whose
    fraction is 0 is the voice above.  One whose fraction is not covers the len_k + 1 samples onset_k .. onset_k + len_k with the terms
    of two_tap_terms over x[s] = f32(row_k[c][s] * g_k) (or row_k[c][s]), each added by a plain f32 add in voice order — the reference's
    Delay by a fraction (the contract of dusp_score_rows_frac_device).  A voice of length 0 takes no part."""
    rows = [np.asarray(r, dtype=np.float32) for r in rows]
    if any(r.ndim != 2 for r in rows):
        raise ValueError("dusp-hip: every row must have shape (channels, samples)")
    n_total = _timeline(n_total)
    if rows:
        n_ch = rows[0].shape[0]
    elif init is not None:
        n_ch = np.asarray(init).shape[0] if np.asarray(init).ndim == 2 else 0
    else:
        n_ch = 1
    if any(r.shape[0] != n_ch for r in rows):
        raise ValueError("dusp-hip: every row must have the same number of channels (%d)" % n_ch)
    onsets = _whole(onsets, len(rows), "onsets")
    return _chain(rows, n_ch, n_total, onsets, _row_lengths(rows, lengths), gains, fracs, init, raw)


def pan_comp(pans):
    """The reference Pan unit's compensation per voice, 10^((1 - |pan|) * 1.5 / 20) (Pan.js:14-16), by the host's pow -> float64 [n]."""
    import math
    return np.array([math.pow(10, ((1 - abs(float(p))) * 1.5) / 20) for p in np.asarray(pans, dtype=np.float32).ravel()], dtype=np.float64)


def _pan_unit(x, p, comp):
    """The reference's Pan unit (Pan.js:21-22) over mono samples x float32 [len], panned to p with the compensation comp -> float32
    [2, len]: float64 operations, each rounded by itself; one rounding to f32"""
    xd, p = x.astype(np.float64), np.float64(p)
    return np.stack([(((xd * (np.float64(1) - p)) / np.float64(2)) * comp).astype(np.float32),
                     (((xd * (np.float64(1) + p)) / np.float64(2)) * comp).astype(np.float32)])


def score_chain_rows_panned(rows, onsets, pans, n_total, lengths=None, gains=None, init=None, raw=False, comp=None, fracs=None):
    """rows: a list of MONO float32 arrays [1, samples_k], onsets int64 [voices], pans float32 [voices] (finite, NOT clamped) -> float32
    [2, n_total]: the contract of dusp_score_rows_pan_device.  It is score_chain_rows with the reference's Pan unit (Pan.js:21-22) applied
    where a voice is added to the timeline: for every timeline sample t

        accL, accR = init[0][t], init[1][t] if init is given else +0, +0
        for k in index order:  s = t - onset_k;  if 0 <= s < len_k:
            x    = f32(row_k[0][s] * g_k) if gains is given else row_k[0][s]
            accL = f32(accL + f32(((f64(x) * (1 - f64(p_k))) / 2) * comp_k))
            accR = f32(accR + f32(((f64(x) * (1 + f64(p_k))) / 2) * comp_k))
        out = acc if raw else (acc || 0)

    every f64 operation rounded by itself.  comp: float64 [voices], None for pan_comp(pans).  Everything else — skipped adds, lengths
    clipped in int64, onsets of any sign, raw partial sums continued through init, windows of the timeline — is score_chain_rows' word for
    word.  It is what the reference renders for Sum.many(Delay(Pan(Multiply(voice_k, g_k), pan_k), onset_k, maxDelay)).

    fracs: as score_chain_rows' (None: today's chain, untouched).  The two taps are applied per channel to the Pan unit's output: the
    f32 left and right values above take the place of x in two_tap_terms — Delay(Pan(Multiply(v, g), p), onset + frac)."""
    rows = [np.asarray(r, dtype=np.float32) for r in rows]
    n = len(rows)
    if any(r.ndim != 2 or r.shape[0] != 1 for r in rows):
        raise ValueError("dusp-hip: every panned row must be mono, of shape (1, samples)")
    n_total = _timeline(n_total)
    onsets = _whole(onsets, n, "onsets")
    with np.errstate(all="ignore"):
        pans = np.asarray(pans, dtype=np.float32)
    if pans.shape != (n,):
        raise ValueError("dusp-hip: pans must have shape (voices=%d,)" % n)
    if not np.all(np.isfinite(pans)):
        raise ValueError("dusp-hip: pans must be finite")
    comp = _comp_array(comp, n, lambda: pan_comp(pans))

    return _chain(rows, 2, n_total, onsets, _row_lengths(rows, lengths), gains, fracs, init, raw, place=lambda k, x: _pan_unit(x[0], pans[k], comp[k]))


def stereo_pans(pans, n):
    """pans of n voices of a stereo piece -> float32 [n], NaN where a voice is not placed: None (nothing placed), or one entry a voice,
    a number or None.  An infinite pan is refused; NaN is "not placed".  Needs no device."""
    if pans is None:
        return np.full(n, np.nan, dtype=np.float32)
    if isinstance(pans, (list, tuple)):
        pans = [np.nan if p is None else p for p in pans]
    with np.errstate(all="ignore"):
        pans = np.ascontiguousarray(pans, dtype=np.float32)
    if pans.shape != (n,):
        raise ValueError("dusp-hip: pans must have shape (voices=%d,)" % n)
    if np.any(np.isinf(pans)):
        raise ValueError("dusp-hip: the pan of voice %d is not finite" % int(np.argmax(np.isinf(pans))))
    return pans


def check_stereo_kinds(channels, pans):
    """channels[k]: the channels of voice k's row, pans: stereo_pans' array.  A voice of a stereo piece is mono or has two channels, and
    only a mono voice is placed: refused by string otherwise."""
    for k, c in enumerate(channels):
        if c not in (1, 2):
            raise ValueError("dusp-hip: a voice of a stereo piece has one or two channels: voice %d has %d" % (k, c))
        if c == 2 and not np.isnan(pans[k]):
            raise ValueError("dusp-hip: a two-channel voice is not panned: the pan of voice %d must be NaN (not placed)" % k)


def score_chain_rows_stereo(rows, onsets, pans, n_total, lengths=None, gains=None, init=None, raw=False, comp=None, fracs=None):
    """rows: a list of float32 arrays [1, samples_k] or [2, samples_k], onsets int64 [voices], pans float32 [voices] with NaN for "not
    placed" (None: nothing placed) -> float32 [2, n_total]: the contract of dusp_score_rows_stereo_device.  The kind of a voice is the
    voice's own: with x_c[s] = f32(row_k[c][s] * g_k) when there are gains and row_k[c][s] otherwise, voice k adds

        mono, finite pan:   f32(((f64(x_0) * (1 - f64(p))) / 2) * comp_k)  left,  the same with 1 + f64(p) right  (score_chain_rows_panned's term, Pan.js:21-22)
        mono, pan NaN:      x_0 left,  x_0 right     (Sum.js:37-38: a mono input feeds every channel of a wider one)
        two channels:       x_0 left,  x_1 right     (its pan must be NaN: Pan's inlet is mono, Pan.js:6)

    Everything else — acc = f32(acc + term) per channel in voice order, no add where a voice does not cover t, init, raw, `acc || 0`,
    lengths clipped in int64, onsets of any sign, windows — is score_chain_rows' word for word, and with fracs the two taps of
    two_tap_terms are applied per channel to the placed values, as score_chain_rows_panned does.  comp: float64 [voices] (None:
    pan_comp(pans); an unplaced voice's is not used).  It is what the reference renders for Sum.many(Delay(P_k, onset_k + frac_k,
    maxDelay)), P_k = Pan(Multiply(v_k, g_k), p_k) for a panned voice and Multiply(v_k, g_k), of one or two channels, otherwise.  All
    voices mono with finite pans gives score_chain_rows_panned's bits, all voices two-channel score_chain_rows'."""
    rows = [np.asarray(r, dtype=np.float32) for r in rows]
    n = len(rows)
    if any(r.ndim != 2 for r in rows):
        raise ValueError("dusp-hip: every row must have shape (channels, samples)")
    n_total = _timeline(n_total)
    onsets = _whole(onsets, n, "onsets")
    pans = stereo_pans(pans, n)
    check_stereo_kinds([r.shape[0] for r in rows], pans)
    comp = _comp_array(comp, n, lambda: pan_comp(np.where(np.isnan(pans), np.float32(0), pans)))

    def place(k, x):
        if x.shape[0] == 2:
            return x
        return np.concatenate([x, x]) if np.isnan(pans[k]) else _pan_unit(x[0], pans[k], comp[k])

    return _chain(rows, 2, n_total, onsets, _row_lengths(rows, lengths), gains, fracs, init, raw, place=place)


# ---- Space placement: a delay and a gain per voice and speaker ----

SPACE_MAX_SPEAKERS = 8
SPACE_MAX_DELAY = 2.0 ** 24
SPEED_OF_SOUND = 343  # metres a second (SpaceChannel.js)


def check_taps(delays, tap_gains, n):
    """The taps of n voices -> contiguous float64 (delays [n, C], gains [n, C]): checked — 1 <= C <= 8 speakers, a finite delay in
    [0, 2^24] samples and a finite gain per voice and speaker — by the strings the C calls use (dusp_score_rows_space_device).  Needs no
    device."""
    with np.errstate(all="ignore"):
        delays = np.ascontiguousarray(delays, dtype=np.float64)
        tap_gains = np.ascontiguousarray(tap_gains, dtype=np.float64)
    if delays.ndim != 2 or delays.shape[0] != n or delays.shape != tap_gains.shape:
        raise ValueError("dusp-hip: the taps' delays and gains must both have shape (voices=%d, speakers)" % n)
    if not 1 <= delays.shape[1] <= SPACE_MAX_SPEAKERS:
        raise ValueError("dusp-hip: a Space has 1 .. %d speakers, not %d" % (SPACE_MAX_SPEAKERS, delays.shape[1]))
    bad = ~np.isfinite(delays)
    if bad.any():
        raise ValueError("dusp-hip: the delay of voice %d at speaker %d is not finite" % tuple(int(i) for i in np.argwhere(bad)[0]))
    bad = (delays < 0) | (delays > SPACE_MAX_DELAY)
    if bad.any():
        raise ValueError("dusp-hip: the delay of voice %d at speaker %d is outside [0, 2^24] samples" % tuple(int(i) for i in np.argwhere(bad)[0]))
    bad = ~np.isfinite(tap_gains)
    if bad.any():
        raise ValueError("dusp-hip: the gain of voice %d at speaker %d is not finite" % tuple(int(i) for i in np.argwhere(bad)[0]))
    return delays, tap_gains


def score_chain_rows_placed(rows, onsets, delays, tap_gains, n_total, lengths=None, gains=None, init=None, raw=False):
    """rows: a list of MONO float32 arrays [1, samples_k], onsets int64 [voices], delays and tap_gains float64 [voices, C] (check_taps)
    -> float32 [C, n_total]: the contract of dusp_score_rows_space_device.  Voice k reaches speaker c through a gain G_kc and a delay of
    D_kc samples, the reference's Gain and MonoDelay units behind the voice: with i = floor(D), fr = D - i (exact in f64), w1 = fr,
    w0 = 1.0 - fr and x[s] the voice's sample after the per-voice gain (f32(row_k[s] * g_k) or row_k[s])

        y_c[s]   = f32(G_kc * f64(x[s]))              (Gain.js:22: one f64 product, one rounding)
        fr == 0:   term(s) = y_c[s], 0 <= s < len, at t = onset_k + i + s
        fr != 0:   two_tap_terms(y_c, fr) over the len + 1 samples from t = onset_k + i
        acc_c    = f32(acc_c + term)                  per channel, in voice index order; no add where a voice does not cover t

    init, raw, `acc || 0`, a voice of length 0, clipping to the timeline and windows (the same chain with onset - lo) are
    score_chain_rows' word for word.  onset_k + i is formed without wrapping (Python integers): a span that leaves int64 lies outside
    every timeline."""
    rows = [np.asarray(r, dtype=np.float32) for r in rows]
    n = len(rows)
    if any(r.ndim != 2 or r.shape[0] != 1 for r in rows):
        raise ValueError("dusp-hip: every placed row must be mono, of shape (1, samples)")
    n_total = _timeline(n_total)
    onsets = _whole(onsets, n, "onsets")
    delays, tap_gains = check_taps(delays, tap_gains, n)
    n_ch = delays.shape[1]
    lengths = _row_lengths(rows, lengths)
    gains = _gains_table(gains, n)
    acc = _chain_start(init, n_ch, n_total)
    with np.errstate(all="ignore"):
        for k, row in enumerate(rows):
            length = int(lengths[k])
            if length == 0:
                continue
            x = row[0, :length]
            if gains is not None:
                x = x * gains[k]  # float32 * float32 scalar: one f32 rounding
            xd = x.astype(np.float64)
            for c in range(n_ch):
                whole = np.floor(delays[k, c])
                frac = delays[k, c] - whole
                onset = int(onsets[k]) + int(whole)
                y = (tap_gains[k, c] * xd).astype(np.float32)
                term = two_tap_terms(y, frac) if frac != 0 else y
                t0, t1 = max(onset, 0), min(onset + len(term), n_total)
                if t1 > t0:
                    acc[c, t0:t1] = acc[c, t0:t1] + term[t0 - onset:t1 - onset]  # float32 + float32: one f32 rounding
    return _chain_end(acc, raw)


def check_places(places, n, speakers=None):
    """places of n voices and the speakers -> float32 (places [n, dims], speakers [C, dims]): 1 to 3 finite coordinates each, the same
    number; speakers None: the reference's stereo pair [[-1, 0], [1, 0]] (Space.js).  Refused by string; needs no device."""
    with np.errstate(all="ignore"):
        try:
            places = np.array(places, dtype=np.float64)
            speakers = np.array([[-1, 0], [1, 0]] if speakers is None else speakers, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("dusp-hip: places and speakers are lists of 1 to 3 coordinates each")
    if places.ndim != 2 or places.shape[0] != n or not 1 <= places.shape[1] <= 3:
        raise ValueError("dusp-hip: places must have shape (voices=%d, 1 .. 3 coordinates)" % n)
    if speakers.ndim != 2 or not 1 <= speakers.shape[1] <= 3:
        raise ValueError("dusp-hip: speakers must have shape (speakers, 1 .. 3 coordinates)")
    if not 1 <= speakers.shape[0] <= SPACE_MAX_SPEAKERS:
        raise ValueError("dusp-hip: a Space has 1 .. %d speakers, not %d" % (SPACE_MAX_SPEAKERS, speakers.shape[0]))
    if speakers.shape[1] != places.shape[1]:
        raise ValueError("dusp-hip: places have %d coordinates, speakers have %d: the same number" % (places.shape[1], speakers.shape[1]))
    if not np.all(np.isfinite(places)):
        raise ValueError("dusp-hip: the place of voice %d is not finite" % int(np.argwhere(~np.isfinite(places))[0][0]))
    if not np.all(np.isfinite(speakers)):
        raise ValueError("dusp-hip: the place of speaker %d is not finite" % int(np.argwhere(~np.isfinite(speakers))[0][0]))
    with np.errstate(all="ignore"):
        return places.astype(np.float32), speakers.astype(np.float32)


def space_taps(places, speakers=None, decibels_per_metre=-3, sample_delay_per_metre=None, sample_rate=None):
    """The reference's SpaceChannel (src/patches/SpaceChannel.js) per voice and speaker, with its roundings -> (delays float64 [n, C],
    gains float64 [n, C]), what score_chain_rows_placed and the device take.  Every coordinate and factor is an inlet constant, rounded
    to f32 (Inlet.js:88-91); Subtract, VectorMagnitude and Multiply store f32:

        dx   = f32(p - q) per coordinate          dist = f32(sqrt(sum of f64(dx)^2)), the sum in f64 in coordinate order
        dB   = f32(dist * dBpm)                   D    = f32(dist * f32(sdpm)), sdpm = sample_rate / 343 by default
        G    = pow(10, dB / 20) in f64, by the host's pow (Gain.js)

    places [n][1 .. 3], speakers [C][the same]; speakers None: [[-1, 0], [1, 0]].  A delay the device would refuse (not finite, beyond
    2^24 samples) is refused here, by its string."""
    import math
    places = np.asarray(places)
    places, speakers = check_places(places, places.shape[0] if places.ndim else 0, speakers)
    if sample_delay_per_metre is None:
        if sample_rate is None:
            from . import config
            sample_rate = config.sampleRate
        sample_delay_per_metre = sample_rate / SPEED_OF_SOUND
    f32, f64 = np.float32, np.float64
    with np.errstate(all="ignore"):
        dbpm, sdpm = f32(decibels_per_metre), f32(sample_delay_per_metre)
    if not np.isfinite(dbpm) or not np.isfinite(sdpm):
        raise ValueError("dusp-hip: decibels_per_metre and sample_delay_per_metre are finite numbers")
    n, n_ch = places.shape[0], speakers.shape[0]
    delays, gains = np.zeros((n, n_ch), dtype=f64), np.zeros((n, n_ch), dtype=f64)
    with np.errstate(all="ignore"):
        for k in range(n):
            for c in range(n_ch):
                total = f64(0)
                for p, q in zip(places[k], speakers[c]):
                    dx = f64(f32(f64(p) - f64(q)))
                    total = total + dx * dx
                dist = f32(np.sqrt(total))
                db = f32(f64(dist) * f64(dbpm))
                delays[k, c] = f64(f32(f64(dist) * f64(sdpm)))
                gains[k, c] = math.pow(10, float(db) / 20) if np.isfinite(db) else np.nan
    return check_taps(delays, gains, n)


# ---- the placement of a call's voices: its keywords as one checked thing ----

STEREO_NO_PLACES = "dusp-hip: places and stereo do not go together: a placed voice is mono and the speakers are the channels"
SPACE_ALONE = "dusp-hip: places stand alone: together with pans or fracs they are refused (a sub-sample onset in front of a Space would be a second two-tap stage)"


def pan_arrays(pans, n, comp=None):
    """pans of n voices -> (float32 [n], float64 [n] compensation): checked — one finite pan a voice, not clamped — with the reference Pan
    unit's compensation 10^((1 - |pan|) * 1.5 / 20) by math.pow where comp is None (pan_comp).  Needs no device."""
    with np.errstate(all="ignore"):
        pans = np.ascontiguousarray(pans, dtype=np.float32)
    if pans.shape != (n,):
        raise ValueError("dusp-hip: pans must have shape (voices=%d,)" % n)
    if not np.all(np.isfinite(pans)):
        raise ValueError("dusp-hip: the pan of voice %d is not finite" % int(np.argmax(~np.isfinite(pans))))
    return pans, _comp_array(comp, n, lambda: pan_comp(pans))


def stereo_pan_arrays(pans, n, comp=None):
    """pans of n voices of a stereo piece -> (float32 [n] with NaN for "not placed", float64 [n] compensation): None (nothing placed)
    or one entry a voice, a number, None or NaN; an infinite pan is refused (stereo_pans).  The compensation is pan_arrays'; an
    unplaced voice's is 1 and is not read.  Needs no device."""
    pans = stereo_pans(pans, n)

    def made():
        comp, placed = np.ones(n, dtype=np.float64), ~np.isnan(pans)
        comp[placed] = pan_comp(pans[placed])
        return comp

    return pans, _comp_array(comp, n, made)


def _comp_array(comp, n, made):
    """the compensation of n voices -> float64 [n]: the caller's, checked, or made()"""
    if comp is None:
        return made()
    comp = np.ascontiguousarray(comp, dtype=np.float64)
    if comp.shape != (n,):
        raise ValueError("dusp-hip: comp must have shape (voices=%d,)" % n)
    return comp


frac_arrays = check_fracs  # (the name the hosts know it by)


def tap_arrays(taps, n):
    """taps = (delays, gains) of n voices -> float64 (delays [n, C], gains [n, C]): checked — 1 .. 8 speakers, finite delays in
    [0, 2^24] samples, finite gains — by the strings the library uses (check_taps).  Needs no device."""
    try:
        delays, gains = taps
    except (TypeError, ValueError):
        raise ValueError("dusp-hip: taps are a pair (delays, gains), each of shape (voices=%d, speakers)" % n)
    return check_taps(delays, gains, n)


def check_piece_channels(channels):
    """channels[p]: the output channels of part p's circuit.  A piece has one channel count: refused by string otherwise."""
    for p, c in enumerate(channels):
        if c != channels[0]:
            raise DuspError("dusp-hip: the voices of a piece must have one number of output channels: part %d has %d, part 0 has %d" % (p, c, channels[0]))
    return channels[0]


def check_pan_channels(channels):
    """channels[p]: the output channels of part p's circuit.  A panned voice is mono: refused by string otherwise."""
    for p, c in enumerate(channels):
        if c != 1:
            raise DuspError("dusp-hip: a panned voice is mono: part %d has %d output channels" % (p, c))
    return 2


def check_space_channels(channels, speakers):
    """channels[p]: the output channels of part p's circuit.  A placed voice is mono: refused by string otherwise."""
    for p, c in enumerate(channels):
        if c != 1:
            raise DuspError("dusp-hip: a placed voice is mono: part %d has %d output channels" % (p, c))
    return speakers


def check_stereo_channels(channels, part_of, pans):
    """channels[p]: the output channels of part p's circuit; part_of[k]: voice k's part; pans: float32 with NaN for "not placed".  A
    voice of a stereo piece has one or two channels, and one of two is not placed: refused by string otherwise."""
    check_stereo_kinds([channels[p] for p in part_of], pans)
    return 2


class Placement:
    """How the n voices of a score or piece are placed where they are added to the timeline: the keywords of a call — pans (with comp),
    fracs, taps = (delays, gains) or, at sample_rate, a space = (places, speakers, decibels_per_metre, sample_delay_per_metre), and
    stereo — checked once, by the strings the library uses.  Needs no device.
        kind    "rows", "pan", "space" or "stereo": which chain the voices are held to (chain) and which entry of the library renders them
        pans    float32 [n] — stereo: with NaN for a voice that is not placed — and comp, float64 [n]; both None without pans
        fracs   float64 [n], or None
        taps    (delays, gains), float64 [n, speakers] each, or None
    fracs_first: the fractions are looked at before the pans, Context.render_score_parts' order of refusal (a piece's is pans first)."""

    def __init__(self, n, pans=None, comp=None, fracs=None, taps=None, stereo=False, space=None, sample_rate=None, fracs_first=False):
        self.refuse_together(pans, fracs, taps if space is None else space, stereo)
        self.kind = "stereo" if stereo else "space" if taps is not None or space is not None else "pan" if pans is not None else "rows"
        self.pans = self.comp = self.fracs = self.taps = None
        if fracs is not None and fracs_first:
            self.fracs = frac_arrays(fracs, n)
        if stereo:
            self.pans, self.comp = stereo_pan_arrays(pans, n, comp)
        elif pans is not None:
            self.pans, self.comp = pan_arrays(pans, n, comp)
        if fracs is not None and not fracs_first:
            self.fracs = frac_arrays(fracs, n)
        if space is not None:
            check_places(space[0], n, space[1])
            self.taps = space_taps(*space, sample_rate=sample_rate)
        elif taps is not None:
            self.taps = tap_arrays(taps, n)

    @staticmethod
    def refuse_together(pans, fracs, places, stereo):
        """what does not go together, refused before anything else of a call is looked at (places: taps or a space, whichever the call has)"""
        if places is not None and stereo:
            raise ValueError(STEREO_NO_PLACES)
        if places is not None and (pans is not None or fracs is not None):
            raise ValueError(SPACE_ALONE)

    def keywords(self):
        """-> the keywords of Context.render_score_parts that say the same"""
        return dict(pans=self.pans, fracs=self.fracs, taps=self.taps, stereo=self.kind == "stereo")

    def channels(self, voice_channels):
        """the timeline's channels where a voice has voice_channels, unchecked: voices that do not fit are the library's to refuse"""
        return self.taps[0].shape[1] if self.kind == "space" else voice_channels if self.kind == "rows" else 2

    def timeline_channels(self, part_channels, part_of):
        """part_channels[p]: the output channels of part p's circuit; part_of[k]: voice k's part -> the timeline's channels; parts that
        do not fit the placement are refused by string"""
        if self.kind == "stereo":
            return check_stereo_channels(part_channels, part_of, self.pans)
        if self.kind == "space":
            return check_space_channels(part_channels, self.channels(1))
        return check_pan_channels(part_channels) if self.kind == "pan" else check_piece_channels(part_channels)

    @property
    def chain(self):
        """the contract the placed voices are held to, which takes the arrays held here beside the rows and onsets"""
        return {"rows": score_chain_rows, "pan": score_chain_rows_panned, "space": score_chain_rows_placed, "stereo": score_chain_rows_stereo}[self.kind]


# ---- the master of a score or piece: one mono circuit over every channel of the timeline ----

MASTER_INPUT_ALONE = "dusp-hip: a MasterInput carries no samples: it stands for the timeline inside the master of a score or piece"
MASTER_NOT_CALLABLE = "dusp-hip: master is a function fx(x) of the mix, or a list of one function a channel of the timeline"
MASTER_COUNT = "dusp-hip: master lists %d circuits, the timeline has %d channels: one a channel"
MASTER_ONE_INPUT = "dusp-hip: the master of channel %d holds %d MasterInput units: a master reads the mix through exactly one, the one it is given"
MASTER_HOST_SOURCE = "dusp-hip: the master of channel %d holds a HostSource: the timeline is a master's only input"
MASTER_EVENTS = "dusp-hip: the master of channel %d has scheduled events: a master is rendered in one piece"
MASTER_CHANNELS = "dusp-hip: the master of channel %d has %d output channels: a master is a mono circuit, applied to every channel by itself"
MASTER_NOT_ISOMORPHIC = "dusp-hip: the masters of channels 0 and %d are not isomorphic circuits: they are one program and may differ in constants only"
MASTER_RATE = "dusp-hip: the master's sample rate is %d, the voices' is %d"


def master_chain(raw, render_channel):
    """The master stage of a score or piece, over its raw timeline: the contract of dusp_render_host_score_piece with a master, needs no
    GPU.  raw float32 [channels, n_total]: the chain's running sums as they stand behind the last voice (score_chain* with raw=True:
    NaN, Inf and -0 kept — in the reference a unit behind a Sum hears the Sum's own values, `|| 0` is renderChannelData's copy-out's).
    render_channel(c, samples) -> float32 [n_total]: the render of the master's instance c over n_total samples from its initial
    state with `samples`, float32 [n_total], as its one input stream, `|| 0` applied at ITS copy-out as every render does (the tests
    pass the CPU oracle).  -> float32 [channels, n_total]: channel c is render_channel(c, raw[c]); no channel hears another."""
    raw = np.asarray(raw)
    if raw.dtype != np.float32 or raw.ndim != 2:
        raise ValueError("dusp-hip: the raw timeline is float32 of shape (channels, n_total)")
    out = np.empty_like(raw)
    for c in range(raw.shape[0]):
        y = np.asarray(render_channel(c, np.ascontiguousarray(raw[c])), dtype=np.float32)
        if y.shape != (raw.shape[1],):
            raise ValueError("dusp-hip: the master's render of channel %d must have shape (n_total=%d,)" % (c, raw.shape[1]))
        out[c] = y
    return out


# ---- effect sends: per-voice levels into bus circuits beside the dry mix ----

BUS_MAX = 4
BUS_NOT_CALLABLE = "dusp-hip: bus %d is a function fx(x) of its send timeline, or a list of one function a channel of the timeline"
BUS_CIRCUITS = "dusp-hip: bus %d lists %d circuits, the timeline has %d channels: one a channel"
BUS_ONE_INPUT = "dusp-hip: bus %d, channel %d, holds %d MasterInput units: a bus reads its sends through exactly one, the one it is given"
BUS_HOST_SOURCE = "dusp-hip: bus %d, channel %d, holds a HostSource: the send timeline is a bus's only input"
BUS_EVENTS = "dusp-hip: bus %d, channel %d, has scheduled events: a bus is rendered in one piece"
BUS_CHANNELS = "dusp-hip: bus %d, channel %d, has %d output channels: a bus is a mono circuit, applied to every channel by itself"
BUS_NOT_ISOMORPHIC = "dusp-hip: the circuits of bus %d at channels 0 and %d are not isomorphic: they are one program and may differ in constants only"
BUS_RATE = "dusp-hip: the sample rate of bus %d is %d, the voices' is %d"
SENDS_WITHOUT_BUSES = "dusp-hip: sends without buses: a send level is what a voice gives to a bus"
BUSES_WITHOUT_SENDS = "dusp-hip: buses without sends: every bus needs a send level a voice (sends of shape (buses, voices))"
BUS_COUNT = "dusp-hip: a call has 1 .. 4 buses, not %d"
SENDS_PLACEMENT = "dusp-hip: sends go with plain rows and with pans at whole-sample onsets: together with fracs, places or stereo they are refused"
SENDS_SHAPE = "dusp-hip: sends must have shape (buses=%d, voices=%d)"
SENDS_NOT_FINITE = "dusp-hip: the send level of voice %d into bus %d is not finite"


def check_sends(sends, n, n_buses):
    """the send levels of n voices into n_buses buses -> contiguous float32 [n_buses, n]: one finite level a bus and voice; a 1-D array
    of n levels is accepted for one bus.  Refused by the strings the library uses: a number of buses outside 1 .. 4, another shape, a
    level that is not finite as float32.  Needs no device."""
    if not 1 <= n_buses <= BUS_MAX:
        raise ValueError(BUS_COUNT % n_buses)
    with np.errstate(all="ignore"):
        sends = np.asarray(sends, dtype=np.float32)
    if sends.ndim == 1 and n_buses == 1:
        sends = sends.reshape(1, -1)
    if sends.shape != (n_buses, n):
        raise ValueError(SENDS_SHAPE % (n_buses, n))
    sends = np.ascontiguousarray(sends)
    if not np.all(np.isfinite(sends)):
        b, k = np.argwhere(~np.isfinite(sends))[0]
        raise ValueError(SENDS_NOT_FINITE % (int(k), int(b)))
    return sends


def refuse_sends_placement(fracs, places, stereo):
    """what sends do not go with, refused on every surface before anything renders"""
    if fracs is not None or places is not None or stereo:
        raise ValueError(SENDS_PLACEMENT)


def score_chain_sends(rows, onsets, n_total, sends, lengths=None, gains=None, pans=None, comp=None):
    """The chain of a score or piece with effect sends: the contract of dusp_score_rows_send_device, needs no GPU.  rows, onsets,
    lengths, gains: as score_chain_rows takes them, or — with pans (and comp) — as score_chain_rows_panned does (mono rows, two
    channels); sends: float32 [B, voices], 1 <= B <= 4 (check_sends) -> (dry_raw float32 [C, n_total], send_raw float32 [B, C, n_total]).

        dry[c][t]    : score_chain_rows / score_chain_rows_panned with raw=True, untouched
        send_b[c][t] = +0; for k in index order, where voice k covers t:
                           send_b = f32(send_b + f32(dry_term_k[c][t] * sends[b][k]))

    dry_term_k[c][t] is exactly the f32 value the dry chain adds for voice k at channel c — the row's sample, f32(row * g_k), or the
    Pan unit's two f32 values — so a send is post-fader and post-pan: Multiply(Multiply(Delay(v_k, onset_k), g_k), s_bk) in the
    reference, for a panned voice behind its Pan.  The product and the add are plain f32 operations, each rounded by itself: the send
    term is f32(f32(x * g) * s), never f32(x * (g * s)).

    EVERY voice is in EVERY bus's chain: a level of 0 is a multiplication by 0, as the reference's would be, and there is no skipped
    add — NaN * 0 poisons the bus where the voice sounds, and -x * 0 is -0.  Both timelines are raw: NaN, Inf and -0 kept."""
    rows = [np.asarray(r, dtype=np.float32) for r in rows]
    if sends is None:
        raise ValueError(BUSES_WITHOUT_SENDS)
    s = np.asarray(sends)
    sends = check_sends(s, len(rows), 1 if s.ndim == 1 else s.shape[0])
    if pans is not None:
        dry = score_chain_rows_panned(rows, onsets, pans, n_total, lengths, gains, None, True, comp)  # (its checks, in its order)
        pans = np.asarray(pans, dtype=np.float32)
        comp = _comp_array(comp, len(rows), lambda: pan_comp(pans))
        both = _chain(rows, 2, _timeline(n_total), _whole(onsets, len(rows), "onsets"), _row_lengths(rows, lengths), gains, None, None, True,
                      place=lambda k, x: _pan_unit(x[0], pans[k], comp[k]), sends=sends)
    else:
        dry = score_chain_rows(rows, onsets, n_total, lengths, gains, None, True)
        both = _chain(rows, dry.shape[0], _timeline(n_total), _whole(onsets, len(rows), "onsets"), _row_lengths(rows, lengths), gains, None, None, True, sends=sends)
    assert dry.tobytes() == both[0].tobytes()  # (the dry half IS today's chain)
    return dry, both[1]


def bus_return(dry_raw, wets, raw=False):
    """The return of the buses onto the dry mix: dry_raw float32 [C, n_total] (the raw dry timeline), wets a list of B float32
    [C, n_total] (bus b's render over its raw send timeline: master_chain(send_raw[b], ...), `|| 0` applied at the bus's own copy-out)
    -> float32 [C, n_total]:

        mix = f32(...f32(f32(dry + wet_0) + wet_1)... + wet_{B-1})        (Sum.many([dry, wet_0, ...]): left-deep, one rounding an add)

    and `mix || 0` unless raw (raw: what a master behind the buses reads).  One divergence from the reference's one circuit comes
    from rendering a bus as a program of its own: where a bus's output is NaN its copy-out has made it 0 already, so the dry sample
    survives, where the reference's final Sum would be NaN and leave as 0."""
    dry_raw = np.asarray(dry_raw)
    if dry_raw.dtype != np.float32 or dry_raw.ndim != 2:
        raise ValueError("dusp-hip: the raw timeline is float32 of shape (channels, n_total)")
    acc = dry_raw.copy()
    with np.errstate(all="ignore"):
        for b, wet in enumerate(wets):
            wet = np.asarray(wet, dtype=np.float32)
            if wet.shape != dry_raw.shape:
                raise ValueError("dusp-hip: the output of bus %d must have shape (channels=%d, n_total=%d)" % ((b,) + dry_raw.shape))
            acc = acc + wet
    return _chain_end(acc, raw)


# ---- tracks: sub-mixes of a piece through insert circuits ----

TRACK_MAX = 8
TRACK_NOT_CALLABLE = "dusp-hip: track %d is None (a fader group), a function fx(x) of its sub-mix, or a list of one function a channel of the timeline"
TRACK_CIRCUITS = "dusp-hip: track %d lists %d circuits, the timeline has %d channels: one a channel"
TRACK_ONE_INPUT = "dusp-hip: track %d, channel %d, holds %d MasterInput units: a track reads its sub-mix through exactly one, the one it is given"
TRACK_HOST_SOURCE = "dusp-hip: track %d, channel %d, holds a HostSource: the track's timeline is its circuit's only input"
TRACK_EVENTS = "dusp-hip: track %d, channel %d, has scheduled events: a track is rendered in one piece"
TRACK_CHANNELS = "dusp-hip: track %d, channel %d, has %d output channels: a track's circuit is mono, applied to every channel by itself"
TRACK_NOT_ISOMORPHIC = "dusp-hip: the circuits of track %d at channels 0 and %d are not isomorphic: they are one program and may differ in constants only"
TRACK_RATE = "dusp-hip: the sample rate of track %d is %d, the voices' is %d"
TRACKS_WITHOUT_TRACK_OF = "dusp-hip: tracks without track_of: every voice goes to a track or, with -1, straight to the mix"
TRACKS_TRACK_OF_ALONE = "dusp-hip: track_of without tracks: a track is what a voice goes to"
TRACKS_NEED_TRACKS = "dusp-hip: %s without tracks: it says something about every track"
TRACKS_COUNT = "dusp-hip: a call has 1 .. 8 tracks, not %d"
TRACKS_TRACK_OF_SHAPE = "dusp-hip: track_of must have shape (voices=%d,) and hold whole numbers"
TRACKS_TRACK_OF_RANGE = "dusp-hip: voice %d names track %d of %d: track_of holds -1 (straight to the mix) or a track, 0 .. %d"
TRACKS_FADERS_SHAPE = "dusp-hip: faders must have shape (tracks=%d,)"
TRACKS_FADER_NOT_FINITE = "dusp-hip: the fader of track %d is not finite"
TRACKS_SENDS_SHAPE = "dusp-hip: track_sends must have shape (buses=%d, tracks=%d)"
TRACKS_LEVEL_NOT_FINITE = "dusp-hip: the level of track %d into bus %d is not finite"
TRACKS_SENDS_WITHOUT_BUSES = "dusp-hip: track_sends without buses: a level is what a track gives to a bus"
TRACKS_BUSES_WITHOUT_SENDS = "dusp-hip: buses without track_sends: with tracks every bus needs a level a track (track_sends of shape (buses, tracks))"
TRACKS_WITH_SENDS = "dusp-hip: sends and tracks do not go together: with tracks the buses are fed by track_sends, a level a track"


def check_tracks(n, n_tracks, track_of, faders=None, track_sends=None, n_buses=0, sends=None):
    """What says where the n voices of a call with n_tracks tracks go, and what the tracks give -> (track_of int32 [n], faders float32
    [n_tracks] or None, track_sends float32 [n_buses, n_tracks] or None), contiguous.  n_tracks None: the call has no `tracks=`, and
    every other keyword of theirs is refused.  n_buses: the call's buses (0: none); sends: its per-voice `sends=`, which do not go
    with tracks.  Refused by the strings the library uses, in this order: a keyword without tracks; tracks without track_of; a number of
    tracks outside 1 .. 8; another shape of track_of or an entry that is no whole number; an entry outside -1 .. n_tracks - 1 (the voice
    named); another shape of faders; a fader that is not finite as float32 (the track named); sends together with tracks; track_sends
    without buses and buses without track_sends; another shape; a level that is not finite (bus and track named).  Needs no device."""
    if n_tracks is None:
        if track_of is not None:
            raise ValueError(TRACKS_TRACK_OF_ALONE)
        for name, value in (("faders", faders), ("track_sends", track_sends)):
            if value is not None:
                raise ValueError(TRACKS_NEED_TRACKS % name)
        return None, None, None
    if track_of is None:
        raise ValueError(TRACKS_WITHOUT_TRACK_OF)
    if not 1 <= n_tracks <= TRACK_MAX:
        raise ValueError(TRACKS_COUNT % n_tracks)
    of = np.asarray(track_of)
    if of.shape != (n,) or (of.dtype.kind not in "iu" and (of.dtype.kind != "f" or not np.all(np.isfinite(of)) or np.any(of != np.floor(of)))):
        raise ValueError(TRACKS_TRACK_OF_SHAPE % n)
    of = of.astype(np.int64)
    wrong = (of < -1) | (of >= n_tracks)
    if wrong.any():
        k = int(np.argmax(wrong))
        raise ValueError(TRACKS_TRACK_OF_RANGE % (k, int(of[k]), n_tracks, n_tracks - 1))
    of = np.ascontiguousarray(of, dtype=np.int32)
    if faders is not None:
        with np.errstate(all="ignore"):
            faders = np.ascontiguousarray(faders, dtype=np.float32)
        if faders.shape != (n_tracks,):
            raise ValueError(TRACKS_FADERS_SHAPE % n_tracks)
        if not np.all(np.isfinite(faders)):
            raise ValueError(TRACKS_FADER_NOT_FINITE % int(np.argmax(~np.isfinite(faders))))
    if sends is not None:
        raise ValueError(TRACKS_WITH_SENDS)
    if track_sends is not None and not n_buses:
        raise ValueError(TRACKS_SENDS_WITHOUT_BUSES)
    if n_buses and track_sends is None:
        raise ValueError(TRACKS_BUSES_WITHOUT_SENDS)
    if track_sends is not None:
        if not 1 <= n_buses <= BUS_MAX:
            raise ValueError(BUS_COUNT % n_buses)
        with np.errstate(all="ignore"):
            track_sends = np.asarray(track_sends, dtype=np.float32)
        if track_sends.ndim == 1 and n_buses == 1:
            track_sends = track_sends.reshape(1, -1)
        if track_sends.shape != (n_buses, n_tracks):
            raise ValueError(TRACKS_SENDS_SHAPE % (n_buses, n_tracks))
        track_sends = np.ascontiguousarray(track_sends)
        if not np.all(np.isfinite(track_sends)):
            b, g = np.argwhere(~np.isfinite(track_sends))[0]
            raise ValueError(TRACKS_LEVEL_NOT_FINITE % (int(g), int(b)))
    return of, faders, track_sends


def track_mix(direct, ys, faders=None, track_sends=None):
    """The mix of a piece's tracks: the contract of dusp_score_tracks_mix_device and of the stage of dusp_render_host_score_piece_tracks
    behind its track renders, needs no GPU.  direct: float32 [C, n_total], the raw chain over the voices that go straight to the mix
    (zeros where there are none); ys: a list of T float32 [C, n_total], track g's output — master_chain(raw sub_g, ...) where the track
    has a circuit (`|| 0` applied at the circuit's own copy-out), the raw sub-mix sub_g where it has none (NaN, Inf and -0 kept);
    faders: float32 [T] or None; track_sends: float32 [B, T] or None -> (mix float32 [C, n_total], feeds float32 [B, C, n_total]), both
    raw (bus_return makes `|| 0` of the mix, or hands it raw to the master):

        term_g = faders given ? f32(y_g * f_g) : y_g
        mix    = direct; for g in order: mix = f32(mix + term_g)                                  (left-deep, one rounding an add)
        feed_b = +0;     for g in order: feed_b = f32(feed_b + f32(term_g * track_sends[b][g]))

    EVERY track is in EVERY bus's chain: a level of 0 is a multiplication by 0, as in score_chain_sends — NaN * 0 poisons the feed and
    -x * 0 is -0.  A track without a circuit passes a NaN on; a track with one has none to pass (its copy-out made it 0)."""
    direct = np.asarray(direct)
    if direct.dtype != np.float32 or direct.ndim != 2:
        raise ValueError("dusp-hip: the raw timeline is float32 of shape (channels, n_total)")
    ys = [np.asarray(y, dtype=np.float32) for y in ys]
    _, faders, track_sends = check_tracks(0, len(ys), np.zeros(0, dtype=np.int32), faders, track_sends, 0 if track_sends is None else (1 if np.ndim(track_sends) == 1 else len(track_sends)))
    acc = direct.copy()
    feeds = np.zeros((0 if track_sends is None else track_sends.shape[0],) + direct.shape, dtype=np.float32)
    terms = track_terms(ys, faders)
    with np.errstate(all="ignore"):
        for g, y in enumerate(ys):
            if y.shape != direct.shape:
                raise ValueError("dusp-hip: the output of track %d must have shape (channels=%d, n_total=%d)" % ((g,) + direct.shape))
            term = terms[g]
            acc = acc + term
            for b in range(feeds.shape[0]):
                feeds[b] = feeds[b] + term * track_sends[b, g]
    return acc, feeds


# ---- stems: the direct mix, every track and every bus return beside the mix ----

STEMS_NOT_BOOL = "dusp-hip: stems is True or False: with True a call delivers the direct mix, every track and every bus return beside the mix"


def check_stems(stems):
    """`stems=` of a score or piece call -> bool; what is no bool is refused by string (a list of names, a count: later changes)"""
    if not isinstance(stems, (bool, np.bool_)):
        raise ValueError(STEMS_NOT_BOOL)
    return bool(stems)


def stem_names(n_tracks, n_buses):
    """the names of the S + 1 signals of a call with stems, in the order they are delivered: direct, track0 .., bus0 .., mix"""
    return ["direct"] + ["track%d" % g for g in range(n_tracks)] + ["bus%d" % b for b in range(n_buses)] + ["mix"]


def track_terms(ys, faders=None):
    """What every track adds to the mix, as track_mix forms it: ys a list of T float32 arrays, faders float32 [T] or None -> a list of T
    float32 arrays, term_g = faders given ? f32(y_g * f_g) : y_g — raw: NaN, Inf and -0 kept.  The faders are held as check_tracks
    holds them."""
    ys = [np.asarray(y, dtype=np.float32) for y in ys]
    if faders is None or not ys:
        return ys
    _, faders, _ = check_tracks(0, len(ys), np.zeros(0, dtype=np.int32), faders)
    with np.errstate(all="ignore"):
        return [y * faders[g] for g, y in enumerate(ys)]


def stems(direct_raw, terms, wets, out):
    """The signals of a call with stems: the contract of dusp_render_host_score_piece_stems, needs no GPU.  direct_raw: float32
    [C, n_total], the raw chain over the voices that go straight to the mix (with tracks), or the raw dry chain over all voices
    (without); terms: track_terms' list of T; wets: a list of B float32 [C, n_total], every bus's render as its own copy-out left it
    (`|| 0` applied there); out: the call's output as it is without stems, behind the master where there is one
    -> float32 [S + 1, C, n_total], S = 1 + T + B, named by stem_names(T, B):

        0           direct || 0
        1 .. T      term_g || 0
        T+1 .. T+B  wet_b
        S           out

    `|| 0`: NaN -> +0 and -0 -> +0.  The stems are in front of the master.  THE PROPERTY THAT MAKES THESE STEMS: in a call without a
    master whose raw signals hold no NaN, or0(f32(...f32(f32(stem_0 + stem_1) + stem_2)... + stem_{S-1})), left-deep in this order, is
    `out` bit for bit — `|| 0` on a stem only changes the sign of a zero, which changes a sum only where the sum is a zero, and the
    last `|| 0` removes that.  A NaN breaks it: a fader group (a track without a circuit) passes a NaN of its voices on, its stem is
    0 there and the mix is 0 there, but the other stems add up to something else."""
    direct_raw = np.asarray(direct_raw)
    if direct_raw.dtype != np.float32 or direct_raw.ndim != 2:
        raise ValueError("dusp-hip: the raw timeline is float32 of shape (channels, n_total)")
    signals = [_chain_end(direct_raw, False)]
    for name, group, raw in (("track", terms, False), ("bus", wets, True)):
        for j, x in enumerate(group):
            x = np.asarray(x, dtype=np.float32)
            if x.shape != direct_raw.shape:
                raise ValueError("dusp-hip: the output of %s %d must have shape (channels=%d, n_total=%d)" % ((name, j) + direct_raw.shape))
            signals.append(_chain_end(x, raw))
    out = np.asarray(out, dtype=np.float32)
    if out.shape != direct_raw.shape:
        raise ValueError("dusp-hip: the mix must have shape (channels=%d, n_total=%d)" % direct_raw.shape)
    signals.append(out)
    return np.stack(signals)


def stems_sum(stack):
    """or0 of the left-deep f32 sum of the stems of a stack (all but its last signal): what stems' property compares with the mix"""
    acc = np.asarray(stack[0], dtype=np.float32).copy()
    with np.errstate(all="ignore"):
        for x in stack[1:-1]:
            acc = acc + np.asarray(x, dtype=np.float32)
    return _chain_end(acc, False)


# ---- meters: RMS and ITU-R BS.1770-4 loudness of the mix and of every stem ----

METERS_NOT_BOOL = "dusp-hip: meters is True or False: with True a call also delivers the RMS and the BS.1770 loudness of every signal it delivers"
METER_RATE_MIN = 8000  # (the shelf's tan needs sample_rate > 2 * 1682 Hz; 8000 is the lowest rate the project tests)
METER_RATE_LOW = "dusp-hip: meters need a sample rate of at least 8000 Hz, not %d: the K-weighting's shelf lies at 1682 Hz"
LUFS_OFFSET, LUFS_ABSOLUTE_GATE, LUFS_RELATIVE_GATE = -0.691, -70.0, -10.0


def check_meters(meters):
    """`meters=` of a score or piece call -> bool; what is no bool is refused by string, as stems= is"""
    if not isinstance(meters, (bool, np.bool_)):
        raise ValueError(METERS_NOT_BOOL)
    return bool(meters)


def k_weighting(sample_rate):
    """The K-weighting of ITU-R BS.1770-4 at any sample rate: two biquad sections (b0, b1, b2, a1, a2) in f64, the high shelf and the
    RLB high-pass, by the bilinear re-derivation libebur128 uses; at 48 kHz the standard's table to its last printed digit."""
    import math
    fs = float(sample_rate)
    if not fs >= METER_RATE_MIN:
        raise ValueError(METER_RATE_LOW % sample_rate)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = math.pow(10.0, G / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    shelf = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    den = 1.0 + K / Q + K * K
    rlb = (1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / den, (1.0 - K / Q + K * K) / den)
    return shelf, rlb


def meter_hop(sample_rate):
    """100 ms as a whole number of samples (libebur128's rule); a block is four of them"""
    return (int(sample_rate) + 5) // 10


def meter_blocks(n, sample_rate):
    """how many 400 ms blocks, 100 ms apart, lie in n samples (dusp_meter_blocks)"""
    hop = meter_hop(sample_rate)
    block = 4 * hop
    return 0 if n < block else (n - block) // hop + 1


def k_weighted(rows, sample_rate):
    """rows float32 or float64 [R, n] -> float64 [R, n]: every row through both sections of k_weighting from rest, each section direct
    form I, y = b0 x + b1 x1 + b2 x2 - a1 y1 - a2 y2 left to right, every operation rounded by itself in f64.  THE sequential loop the
    device's cut in time is held to."""
    rows = np.asarray(rows, dtype=np.float64)
    if rows.ndim != 2:
        raise ValueError("dusp-hip: the rows to weight have shape (rows, samples)")
    (b0, b1, b2, a1, a2), (c0, c1, c2, d1, d2) = k_weighting(sample_rate)
    out = np.empty_like(rows)
    if rows.shape[0] >= 16:  # (many rows: one numpy operation a step over all of them — the same operations in the same order)
        r = rows.shape[0]
        x1, x2, y1, y2, z1, z2 = (np.zeros(r) for _ in range(6))
        cols = np.ascontiguousarray(rows.T)
        res = np.empty_like(cols)
        with np.errstate(all="ignore"):
            for t in range(cols.shape[0]):
                x = cols[t]
                y = b0 * x + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
                z = c0 * y + c1 * y1 + c2 * y2 - d1 * z1 - d2 * z2
                x2, x1, y2, y1, z2, z1 = x1, x, y1, y, z1, z
                res[t] = z
        return np.ascontiguousarray(res.T)
    for k in range(rows.shape[0]):  # (few rows: Python's own doubles, which round every operation by itself as well)
        x1 = x2 = y1 = y2 = z1 = z2 = 0.0
        zs = []
        for x in rows[k].tolist():
            y = b0 * x + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            z = c0 * y + c1 * y1 + c2 * y2 - d1 * z1 - d2 * z2
            x2, x1, y2, y1, z2, z1 = x1, x, y1, y, z1, z
            zs.append(z)
        out[k] = zs
    return out


def loudness(e):
    """energies float64 [n_blocks] -> (momentary float64 [n_blocks], lufs): momentary = -0.691 + 10 log10(e), -inf for 0; lufs the
    gated integrated loudness of BS.1770-4 — the blocks above -70, then above their mean's loudness - 10 as well; -inf when no block
    is left, NaN as soon as one energy is not finite.  (What dusp_meter_host computes from the hop sums, in the library.)"""
    e = np.asarray(e, dtype=np.float64)
    with np.errstate(all="ignore"):
        momentary = LUFS_OFFSET + 10.0 * np.log10(e)
        if not np.all(np.isfinite(e)):
            return momentary, float("nan")
        kept = momentary > LUFS_ABSOLUTE_GATE
        if not kept.any():
            return momentary, float("-inf")
        gamma = LUFS_OFFSET + 10.0 * np.log10(np.mean(e[kept])) + LUFS_RELATIVE_GATE
        kept &= momentary > gamma
        if not kept.any():
            return momentary, float("-inf")
        return momentary, float(LUFS_OFFSET + 10.0 * np.log10(np.mean(e[kept])))


def meters(signals, sample_rate):
    """The meters of a delivery: the contract of dusp_meter_host and of meters=True, in f64 throughout, needs no GPU.  signals float32
    [S, C, n] -> dict(rms float64 [S, C], energies float64 [S, n_blocks], momentary float64 [S, n_blocks], lufs float64 [S], hop, block):

        rms[s][c]       sqrt(sum_t f64(x)^2 / n)
        energies[s][j]  sum over c of mean(z_c[j hop : j hop + block]^2), z_c = k_weighted(channel c): EVERY channel has weight 1 —
                        the standard for mono and stereo; a Space timeline's speakers are no 5.1 layout and get weight 1 too
        momentary, lufs loudness(energies[s])

    hop = meter_hop(sample_rate), block = 4 hop, n_blocks = meter_blocks(n, sample_rate).  A block that holds or follows a sample that is
    not finite has an energy that is not finite.  The meters are taken on the f32 signals in front of the PCM gain: the loudness of an
    encoded file is lufs + 20 log10(gain)."""
    signals = np.asarray(signals, dtype=np.float32)
    if signals.ndim != 3:
        raise ValueError("dusp-hip: the signals to meter are float32 of shape (signals, channels, samples)")
    k_weighting(sample_rate)  # (refuses a rate that is too low)
    S, C, n = signals.shape
    hop = meter_hop(sample_rate)
    block, n_blocks = 4 * hop, meter_blocks(n, sample_rate)
    x = signals.astype(np.float64)
    with np.errstate(all="ignore"):
        rms = np.sqrt(np.sum(x * x, axis=2) / n) if n else np.zeros((S, C))
        z = k_weighted(x.reshape(S * C, n), sample_rate).reshape(S, C, n) if n_blocks else x
        energies = np.zeros((S, n_blocks))
        for j in range(n_blocks):
            w = z[:, :, j * hop:j * hop + block]
            energies[:, j] = np.sum(np.mean(w * w, axis=2), axis=1)
    momentary, lufs = np.zeros((S, n_blocks)), np.zeros(S)
    for s in range(S):
        momentary[s], lufs[s] = loudness(energies[s])
    return dict(rms=rms, energies=energies, momentary=momentary, lufs=lufs, hop=hop, block=block)


# ---- loudness delivery: the true peak, and the one gain of a delivery at a loudness target ----

TRUE_PEAK_NOT_BOOL = "dusp-hip: true_peak is True or False: with True a call also delivers the true peak of every signal and channel it delivers"
LOUDNESS_NOT_NUMBER = "dusp-hip: loudness is None or a finite number, the target in LUFS (-14, -16, -23 ...): the frames are then encoded at that loudness"
TRUE_PEAK_MAX_BAD = "dusp-hip: true_peak_max is a finite number of dBTP at most 0 (default -1), the ceiling no delivered signal's true peak exceeds"
LOUDNESS_WITH_NORMALISE = "dusp-hip: loudness and normalise=%d do not go together: the target decides the gain, normalise must be 0"
LOUDNESS_PLANAR = "dusp-hip: loudness goes with the _pcm and _wav calls: 32-bit frames via bit_depth=32 are the f32 delivery at a target"
TRUE_PEAK_TAPS = 49


def check_true_peak(true_peak):
    """`true_peak=` of a score or piece call -> bool; what is no bool is refused by string, as meters= is"""
    if not isinstance(true_peak, (bool, np.bool_)):
        raise ValueError(TRUE_PEAK_NOT_BOOL)
    return bool(true_peak)


def check_loudness(loudness, true_peak_max=-1.0, normalise=0, pcm=True):
    """`loudness=` and `true_peak_max=` of a _pcm or _wav call -> (target in LUFS or None, ceiling in dBTP), floats.  Refused by string:
    a loudness that is no finite number, a ceiling that is not finite or above 0, loudness together with normalise != 0, and loudness
    on a call that delivers planar f32 (pcm False)"""
    def number(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)) and np.isfinite(v)
    if not number(true_peak_max) or true_peak_max > 0:
        raise ValueError(TRUE_PEAK_MAX_BAD)
    if loudness is None:
        return None, float(true_peak_max)
    if not number(loudness):
        raise ValueError(LOUDNESS_NOT_NUMBER)
    if not pcm:
        raise ValueError(LOUDNESS_PLANAR)
    if normalise != 0:
        raise ValueError(LOUDNESS_WITH_NORMALISE % normalise)
    return float(loudness), float(true_peak_max)


def true_peak_taps(sample_rate):
    """The interpolator of the true peak at a sample rate -> (F, h): F = 4 below 96 kHz, 2 below 192 kHz, else 1 — then h = [1.0] and
    the true peak is the sample peak.  F > 1: the windowed sinc libebur128 interpolates with, re-derived here: 49 taps, m = j - 24,
    h[j] = sin(m pi / F) / (m pi / F) — 1 at m = 0, exactly 0 where F divides m — times the Hann window 0.5 (1 - cos(2 pi j / 48)), in
    f64.  Phase p owns h[p::F]: K = ceil(49 / F) taps (13 or 25), a shorter phase padded with a zero tap (dusp_true_peak_taps)."""
    import math
    if not sample_rate > 0:
        raise ValueError("dusp-hip: the true peak needs a sample rate, not %r: it decides the oversampling" % (sample_rate,))
    F = 4 if sample_rate < 96000 else 2 if sample_rate < 192000 else 1
    if F == 1:
        return 1, np.array([1.0])
    h = np.zeros(TRUE_PEAK_TAPS)
    for j in range(TRUE_PEAK_TAPS):
        m = j - 24
        v = 1.0 if m == 0 else 0.0 if m % F == 0 else math.sin(m * math.pi / F) / (m * math.pi / F)
        h[j] = v * (0.5 * (1.0 - math.cos(2.0 * math.pi * j / 48.0)))
    return F, h


def true_peak(signals, sample_rate, taps=None):
    """The true peak of a delivery: the contract of dusp_true_peak_host and of true_peak=True, in f64 throughout, needs no GPU.
    signals float32 [S, C, n] -> float64 [S, C], LINEAR (dBTP is 20 log10).  taps: (F, h) as true_peak_taps makes them (None: its own).

    Per row, x zero outside [0, n): for u in [0, n + K - 1) and every phase p in [0, F), acc = 0.0, then acc = acc + h[p + F k] *
    f64(x[u - k]) for k = 0 .. K - 1 in that order — every product and every sum rounded by itself, no fma, a padded phase's zero tap
    multiplied like the rest.  The peak is the largest |acc| over every u and p, the filter's tail behind the last sample included;
    NaN as soon as any acc is not finite; 0 for n = 0."""
    signals = np.asarray(signals, dtype=np.float32)
    if signals.ndim != 3:
        raise ValueError("dusp-hip: the signals to take the true peak of are float32 of shape (signals, channels, samples)")
    F, h = true_peak_taps(sample_rate) if taps is None else (int(taps[0]), np.asarray(taps[1], dtype=np.float64))
    K = -(-len(h) // F)
    phases = np.zeros((F, K))
    for p in range(F):
        own = h[p::F]
        phases[p, :len(own)] = own
    S, C, n = signals.shape
    if n == 0:
        return np.zeros((S, C))
    x = np.zeros((S * C, n + 2 * (K - 1)))
    x[:, K - 1:K - 1 + n] = signals.reshape(S * C, n).astype(np.float64)
    n_out = n + K - 1
    largest, finite = np.zeros(S * C), np.ones(S * C, dtype=bool)
    with np.errstate(all="ignore"):
        for p in range(F):
            acc = np.zeros((S * C, n_out))
            for k in range(K):
                acc = acc + phases[p, k] * x[:, K - 1 - k:K - 1 - k + n_out]  # (x[u - k]; a product and a sum, each rounded by itself)
            finite &= np.all(np.isfinite(acc), axis=1)
            largest = np.maximum(largest, np.max(np.abs(np.where(np.isfinite(acc), acc, 0.0)), axis=1))
    return np.where(finite, largest, np.nan).reshape(S, C)


def loudness_gain(lufs, true_peaks, target_lufs, ceiling_dbtp):
    """The one gain of a delivery at a loudness target under a true-peak ceiling -> (gain, level): with tp the largest of true_peaks (a
    NaN wins), G = min(10^((target - lufs) / 20), 10^(ceiling / 20) / tp); level = float32(1 / G), the sample magnitude that is
    brought to full scale — what the encoders read as the peak under NORMALISE_FULL — and gain = 1.0 / float64(level), what they
    apply.  Unity, (1.0, float32(1.0)): lufs -inf or NaN; tp 0, NaN or Inf; a level that comes out zero, subnormal or not finite.
    Unity leaves the samples as they are, as pcm_gain leaves an instance whose peak is NaN.  (truepeak_plan.hpp true_peak_loudness_gain.)"""
    import math
    unity = (1.0, np.float32(1.0))
    tps = np.asarray(true_peaks, dtype=np.float64).ravel()
    lufs = float(lufs)
    if math.isnan(lufs) or lufs == -math.inf or tps.size == 0:
        return unity
    tp = float("nan") if np.any(np.isnan(tps)) else float(np.max(tps))
    if not tp > 0.0 or not math.isfinite(tp):
        return unity
    with np.errstate(all="ignore"):
        try:
            by_loudness = math.pow(10.0, (float(target_lufs) - lufs) / 20.0)
        except OverflowError:
            by_loudness = math.inf
        G = min(by_loudness, math.pow(10.0, float(ceiling_dbtp) / 20.0) / tp)
        level = np.float32(np.float64(1.0) / np.float64(G))
    if not np.isfinite(level) or level < np.finfo(np.float32).tiny:
        return unity
    return 1.0 / float(np.float64(level)), level


# ---- the look-ahead true-peak limiter of a delivery at a loudness target ----

LIMITER_NOT_BOOL = "dusp-hip: limiter is True or False: with True a delivery at a loudness target is limited to the true-peak ceiling before the one gain is taken"
LIMITER_NEEDS_LOUDNESS = "dusp-hip: limiter without loudness: the limiter's threshold is the ceiling seen from the loudness target, so it needs loudness="
LIMITER_WINDOW_BAD = "dusp-hip: limiter_window is a finite positive number of seconds (default 0.005), the limiter's look-ahead, attack and release"
LIMITER_WINDOW_LONG = "dusp-hip: limiter_window is %d samples at %d Hz: the limiter's window is at most 4096 samples"
LIMITER_THRESHOLD_BAD = "dusp-hip: the limiter's threshold is a finite number above 0, linear"
LIMITER_WINDOW_SAMPLES = "dusp-hip: the limiter's window is a whole number of samples, 1 .. 4096"
LIMITER_ONE = 1 << 30  # the gain curve's fixed point: 30 fractional bits
LIMITER_WINDOW_MAX = 4096
LIMITER_RELEASE_MAX = 1 << 22
LIMITER_RELEASE_BAD = "dusp-hip: limiter_release is None or a finite positive number of seconds, the time the limiter's gain takes from 0 back to 1"
LIMITER_RELEASE_NEEDS_LIMITER = "dusp-hip: limiter_release without limiter=True: a release is the limiter's"
LIMITER_RELEASE_LONG = "dusp-hip: limiter_release is %d samples at %d Hz: the limiter's release is at most 4194304 samples"
LIMITER_RELEASE_SAMPLES = "dusp-hip: the limiter's release is a whole number of samples, 1 .. 4194304"


def check_limiter(limiter, limiter_window, loudness, sample_rate):
    """`limiter=` and `limiter_window=` of a _pcm or _wav call -> L, the window in samples, max(1, round(window x sample_rate)); 0 for
    limiter=False (the window is then not looked at).  Refused by string: a limiter that is no bool, limiter=True without loudness=,
    a window that is no finite positive number, and one of more than 4096 samples"""
    if not isinstance(limiter, (bool, np.bool_)):
        raise ValueError(LIMITER_NOT_BOOL)
    if not limiter:
        return 0
    if loudness is None:
        raise ValueError(LIMITER_NEEDS_LOUDNESS)
    w = limiter_window
    if not isinstance(w, (int, float, np.integer, np.floating)) or isinstance(w, (bool, np.bool_)) or not np.isfinite(w) or not w > 0:
        raise ValueError(LIMITER_WINDOW_BAD)
    exact = float(w) * float(sample_rate)
    if exact > 2.0 * LIMITER_WINDOW_MAX:  # (far too long, perhaps beyond what int() takes: the text says at most 2^62)
        raise ValueError(LIMITER_WINDOW_LONG % (int(exact) if exact < 2.0 ** 62 else 2 ** 62, sample_rate))
    L = max(1, int(round(float(w) * float(sample_rate))))
    if L > LIMITER_WINDOW_MAX:
        raise ValueError(LIMITER_WINDOW_LONG % (L, sample_rate))
    return L


def check_limiter_release(limiter_release, limiter, sample_rate):
    """`limiter_release=` of a _pcm or _wav call -> R, the release in samples, max(1, round(seconds x sample_rate)); 0 for None.
    Refused by string: a release that is no finite positive number (or a bool), one without limiter=True, and one of more than 2^22
    samples"""
    r = limiter_release
    if r is None:
        return 0
    if not isinstance(r, (int, float, np.integer, np.floating)) or isinstance(r, (bool, np.bool_)) or not np.isfinite(r) or not r > 0:
        raise ValueError(LIMITER_RELEASE_BAD)
    if not (isinstance(limiter, (bool, np.bool_)) and limiter):
        raise ValueError(LIMITER_RELEASE_NEEDS_LIMITER)
    exact = float(r) * float(sample_rate)
    if exact > 2.0 * LIMITER_RELEASE_MAX:
        raise ValueError(LIMITER_RELEASE_LONG % (int(exact) if exact < 2.0 ** 62 else 2 ** 62, sample_rate))
    R = max(1, int(round(exact)))
    if R > LIMITER_RELEASE_MAX:
        raise ValueError(LIMITER_RELEASE_LONG % (R, sample_rate))
    return R


def limiter_threshold(lufs, target_lufs, ceiling_dbtp):
    """T, the true-peak magnitude that the gain of the loudness target brings exactly to the ceiling:
    10^(ceiling / 20) / 10^((target - lufs) / 20), two powers and a division in f64 (limiter_plan.hpp limiter_threshold)."""
    import math

    def power(x):  # (C's pow: what overflows is inf, not an exception)
        try:
            return math.pow(10.0, x)
        except OverflowError:
            return math.inf
    with np.errstate(all="ignore"):
        return float(np.float64(power(float(ceiling_dbtp) / 20.0)) / np.float64(power((float(target_lufs) - float(lufs)) / 20.0)))


def _limiter_taps(sample_rate, taps):
    F, h = true_peak_taps(sample_rate) if taps is None else (int(taps[0]), np.asarray(taps[1], dtype=np.float64))
    K = -(-len(h) // F)
    phases = np.zeros((F, K))
    for p in range(F):
        own = h[p::F]
        phases[p, :len(own)] = own
    return F, K, phases


def limiter_envelope(signals, sample_rate, taps=None):
    """The limiter's envelope: signals float32 [S, C, n] -> e float64 [n], the largest oversampled magnitude of ANY row around sample
    s.  With F, h, K those of true_peak_taps and D = (K - 1) / 2 (6 at F = 4, 12 at F = 2, 0 at F = 1) every row's accumulators
    acc_p[u] are formed exactly as true_peak forms them; e[s] is the largest |acc_p[s + D]| over all rows and phases — the interpolator
    delays by D samples, so these are the F oversampled points that belong to sample s.  An accumulator that is not finite counts as
    0: the limiter does not react to a NaN or Inf sample.  The filter's head (u < D) and tail (u >= n + D) take no part."""
    signals = np.asarray(signals, dtype=np.float32)
    if signals.ndim != 3:
        raise ValueError("dusp-hip: the signals to limit are float32 of shape (signals, channels, samples)")
    F, K, phases = _limiter_taps(sample_rate, taps)
    D = (K - 1) // 2
    S, C, n = signals.shape
    e = np.zeros(n)
    if n == 0 or S * C == 0:
        return e
    x = np.zeros((S * C, n + 2 * (K - 1)))
    x[:, K - 1:K - 1 + n] = signals.reshape(S * C, n).astype(np.float64)
    with np.errstate(all="ignore"):
        for p in range(F):
            acc = np.zeros((S * C, n))
            for k in range(K):  # u = s + D: x[u - k] lies at K - 1 + s + D - k
                acc = acc + phases[p, k] * x[:, K - 1 + D - k:K - 1 + D - k + n]
            e = np.maximum(e, np.max(np.abs(np.where(np.isfinite(acc), acc, 0.0)), axis=0))
    return e


def _limiter_minima(e, threshold, window):
    """-> (q uint32 [n], m int64 [n + L - 1]): limiter_gain's words and their sliding minima, m[j + (L - 1)] = min(q[j .. j + L - 1])"""
    import math
    T, L = float(threshold), int(window)
    if not (T > 0.0 and math.isfinite(T)):
        raise ValueError(LIMITER_THRESHOLD_BAD)
    if L != window or not 1 <= L <= LIMITER_WINDOW_MAX:
        raise ValueError(LIMITER_WINDOW_SAMPLES)
    e = np.asarray(e, dtype=np.float64)
    n = len(e)
    with np.errstate(all="ignore"):
        r = np.where(e > T, T / np.where(e > T, e, 1.0), 1.0)
    q = np.floor(r * float(LIMITER_ONE)).astype(np.uint32)
    a = np.full(n + 2 * (L - 1), LIMITER_ONE, dtype=np.int64)  # a[j] = q[j - (L - 1)]
    a[L - 1:L - 1 + n] = q
    p, step = a.copy(), 1  # p[i] = min(a[i .. i + step - 1]) wherever that window lies inside a
    while 2 * step <= L:
        p[:len(p) - step] = np.minimum(p[:len(p) - step], p[step:])
        step *= 2
    return q, np.minimum(p[:n + L - 1], p[L - step:L - step + n + L - 1])  # m[j'] = min(a[j' .. j' + L - 1]), j' = j + (L - 1)


def _limiter_mean(m, n, L):
    """g[s] = f64(m[s] + .. + m[s + L - 1]) / f64(L x ONE) in m's indexing: the integer sum, one division"""
    c = np.concatenate(([0], np.cumsum(m)))
    total = c[L:L + n] - c[:n]
    return total.astype(np.float64) / float(L * LIMITER_ONE)


def limiter_gain(e, threshold, window):
    """The limiter's gain curve from its envelope -> (g float64 [n], q uint32 [n]).  T = threshold > 0, L = window, 1 .. 4096 samples:
    r[s] = T / e[s] where e[s] > T, else 1 (one f64 division); q[s] = floor(r[s] x 2^30), ONE = 2^30 outside [0, n);
    m[j] = min(q[j .. j + L - 1]) for j in [-(L - 1), n); sum[s] = m[s - L + 1] + .. + m[s], an exact integer; g[s] = f64(sum[s]) /
    f64(L x ONE).  So g[s] <= r[s], exactly — every minimum in the mean holds q[s], and the floor and the integer mean only round down —
    and g[s] is no lower than the smallest r within L samples of s less 2^-30.  The curve reaches a
    peak's gain in a linear attack of L samples and leaves it in a release of L samples."""
    q, m = _limiter_minima(e, threshold, window)
    return _limiter_mean(m, len(q), int(window)), q


def limiter_release_step(release):
    """d = ceil(ONE / R), the most the held curve rises a sample: a gain of 0 is back at 1 after at most R samples.  R is a whole
    number of samples, 1 .. 2^22 (LIMITER_RELEASE_MAX)"""
    R = int(release)
    if R != release or isinstance(release, (bool, np.bool_)) or not 1 <= R <= LIMITER_RELEASE_MAX:
        raise ValueError(LIMITER_RELEASE_SAMPLES)
    return -(-LIMITER_ONE // R)


def limiter_gain_release(e, threshold, window, release):
    """The gain curve with a release of its own -> (g float64 [n], q uint32 [n], held int64 [n + L - 1]; held[j + (L - 1)] is the held
    curve at j).  q and m are limiter_gain's.  R = release, 1 .. 2^22 samples, d = limiter_release_step(R) = ceil(ONE / R).
    held[j] = min(m[j], held[j - 1] + d) for j from -(L - 1) upwards, held[-L] = ONE — in closed form the minimum over i <= j of
    m[i] + d (j - i), which is how it is formed here: d j + the running minimum of m[i] - d i, all in 64-bit integers (no cap at ONE is
    needed: m[j] <= ONE is a member).  sum[s] = held[s - L + 1] + .. + held[s], g[s] = f64(sum[s]) / f64(L x ONE).  Exactly:
      - R = 1: d = ONE, held = m and g is limiter_gain's bit for bit;
      - held <= m, so g[s] <= limiter_gain's g[s] <= r[s];
      - held[j] - held[j - 1] <= d and sum[s] - sum[s - 1] <= L d: the curve rises by at most d / ONE a sample;
      - m[i] + d (j - i) >= ONE once j - i >= ceil(ONE / d): held[j] depends on at most the last ceil(ONE / d) <= R values of m."""
    d = limiter_release_step(release)
    q, m = _limiter_minima(e, threshold, window)
    at = np.arange(len(m), dtype=np.int64) * d  # (below 2^31 x 2^30)
    held = np.minimum.accumulate(m - at) + at if len(m) else m
    return _limiter_mean(held, len(q), int(window)), q, held


def limit(signals, sample_rate, threshold, window, taps=None, release=None):
    """The linked look-ahead limiter: the contract of dusp_limit_host and of limiter=True, in f64 and integers, needs no GPU.
    signals float32 [S, C, n] -> (limited float32 [S, C, n], g float64 [n], reduction): ONE curve g = limiter_gain(limiter_envelope(
    signals)) for every row, limited = f32(f64(x) x g[s]); reduction = min(g), 1.0 exactly where nothing exceeds the threshold (the
    output is then the input bit for bit).  A NaN sample stays a NaN.  release: None, or R in samples — the curve is then
    limiter_gain_release's (the contract of dusp_limit_release_host and of limiter_release=)."""
    signals = np.asarray(signals, dtype=np.float32)
    e = limiter_envelope(signals, sample_rate, taps)
    g = limiter_gain(e, threshold, window)[0] if release is None else limiter_gain_release(e, threshold, window, release)[0]
    with np.errstate(all="ignore"):
        limited = (signals.astype(np.float64) * g).astype(np.float32)
    return limited, g, (float(np.min(g)) if len(g) else 1.0)


def deliver_limited(signals, sample_rate, target_lufs, ceiling_dbtp, window, taps=None, release=None):
    """The whole chain of a delivery with limiter=True over the f32 signals the call delivers (the mix LAST), in f64, needs no GPU: the
    contract of dusp_render_host_score_piece_limiter.  -> dict(signals, meters, true_peak, gain, level, limiter): the signals that are
    encoded (wav.encode_at_level(signals, bit_depth, level) has the bytes), their meters and true peaks, the one gain and its level,
    and the limiter's record — engaged, threshold, window, reduction, lufs_in, true_peak_in.

    First meters, true_peak and loudness_gain as without a limiter.  T = limiter_threshold(lufs of the mix, target, ceiling).  The
    limiter is engaged where that gain is not unity (level != 1), T is finite and above 0, and the largest true peak exceeds T;
    otherwise the delivery is the one without a limiter.  Engaged: limit(signals, T, window), then meters, true_peak and loudness_gain
    again over the limited signals — the ceiling is held by that gain, and what is returned describes the limited signals.
    release: None, or R in samples (limit's); the record then has release=R, else release=0."""
    import math
    signals = np.asarray(signals, dtype=np.float32)
    metered, tps = meters(signals, sample_rate), true_peak(signals, sample_rate, taps)
    gain, level = loudness_gain(metered["lufs"][-1], tps, target_lufs, ceiling_dbtp)
    lufs_in, tp_in = float(metered["lufs"][-1]), (float("nan") if np.any(np.isnan(tps)) else float(np.max(tps)))
    record = dict(engaged=False, threshold=0.0, window=int(window), reduction=1.0, lufs_in=lufs_in, true_peak_in=tp_in, release=0 if release is None else int(release))
    T = record["threshold"] = limiter_threshold(lufs_in, target_lufs, ceiling_dbtp)
    if level != np.float32(1.0) and T > 0.0 and math.isfinite(T) and tp_in > T:
        signals, _, reduction = limit(signals, sample_rate, T, window, taps, release)
        metered, tps = meters(signals, sample_rate), true_peak(signals, sample_rate, taps)
        gain, level = loudness_gain(metered["lufs"][-1], tps, target_lufs, ceiling_dbtp)
        record.update(engaged=True, reduction=reduction)
    return dict(signals=signals, meters=metered, true_peak=tps, gain=gain, level=level, limiter=record)
