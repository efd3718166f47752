"""dusp_amd — MI355X-native offline render path for Dusp graphs.

Host side (this package): graph construction with the reference's constructor
signatures (graph.py), extraction to a flat descriptor (descriptor.py), and the
ctypes binding of the HIP library (runtime.py).  Device side: dusp_amd/csrc/.
"""
from . import config, descriptor, mix, quick, runtime  # noqa: F401
from .descriptor import DuspError  # noqa: F401
from .mix import space_taps, split_onsets  # noqa: F401
from .graph import (Abs, AllPass, Circuit, CircleBuffer, CircleBufferReader, CircleBufferWriter, Clip, CombFilter, DecibelToScaler, Delay,  # noqa: F401
                    Divide, Filter, FixedDelay, FixedMultiply, Gain, MonoDelay, MultiChannelOsc, ReadBackDelay, HardClipAbove, HardClipBelow, Multiply, Osc, PolarityInvert, Pow,
                    Ramp, Repeater, SecondsToSamples, SemitoneToRatio, Subtract, Sum, Unit,
                    AHD, ConcatChannels, CrossFader, HostSource, MasterInput, MidiToFrequency, Pan, PickChannel, Rescale, SampleRateRedux, Shape, Timer, VectorMagnitude)
from .render import ChannelData, Limiter, Metered, Meters, Stems, limit, meter, render_many, render_mix, render_mix_pcm, render_mix_wav, render_piece, render_piece_pcm, render_piece_wav, render_score, render_score_pcm, render_score_wav, renderChannelData, true_peak  # noqa: F401
from .runtime import Context, DuspHipError, Program  # noqa: F401


def configure(sample_rate=None):
    """Set the process-wide sample rate (the reference does this with `--sampleRate=` on argv,
    src/config.js:1,17).  Call before building graphs."""
    if sample_rate is not None:
        config.sampleRate = int(sample_rate)
