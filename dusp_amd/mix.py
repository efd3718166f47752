"""The mix of a batch of voices in `Sum.many`'s chain order: the contract of dusp_mix_device, in numpy (needs no GPU).

The reference's `Sum.many(voices)` is a left-deep chain ((v0 + v1) + v2) + ... of Sum units, each of which stores its result in
a Float32Array (src/components/Sum.js:18-29,33-44): one f32 rounding per add, in index order.  A gain per voice is a Multiply in
front of the chain: one f32 rounding per product (Multiply.js:23-34)."""
import numpy as np


def mix_chain(planar, gains=None, init=None, raw=False):
    """planar float32 [instances, channels, samples] -> float32 [channels, samples].

        acc = init if given else term(0);  acc = f32(acc + term(i)) for the remaining instances in index order
        term(i) = f32(planar[i] * gains[i]) if gains is given else planar[i]

    Without `init` the chain starts from the first voice itself, not from 0 + v0.  raw: the sums as they stand (a partial sum to be
    continued through `init`: NaN and -0 kept); otherwise NaN and -0 become +0, the `x || 0` of renderChannelData.js:44."""
    planar = np.asarray(planar, dtype=np.float32)
    if planar.ndim != 3 or planar.shape[0] < 1:
        raise ValueError("dusp-hip: planar must have shape (instances >= 1, channels, samples)")
    if gains is not None:
        gains = np.asarray(gains, dtype=np.float32)
        if gains.shape != (planar.shape[0],):
            raise ValueError("dusp-hip: gains must have shape (instances=%d,)" % planar.shape[0])
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
        assert acc.dtype == np.float32
        if not raw:
            acc = np.where(np.isnan(acc) | (acc == 0), np.float32(0), acc)
    return acc
