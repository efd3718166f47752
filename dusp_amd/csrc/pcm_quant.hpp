// pcm_quant.hpp — the PCM sample contract: one f32 sample -> a peak-normalised 16- or 24-bit integer (or a scaled f32).
// Host and device: the encode kernels use it (pcm_engine.hip), and tests/native/pcm_quant_check.cpp pins it on the CPU against
// an integer-exact evaluation of the same steps.  dusp_amd/wav.py restates it in numpy and dusp_amd/js/lib/wav.js in JavaScript
// (`Math.max(-1, Math.min(1, x)) * 32767`, rounded half away from zero, `|| 0` for NaN): all of them produce the same bytes.
//
//   t = (double)x * g          one IEEE multiply (g: the instance's gain, 1 without normalisation)
//   t = NaN ? 0 : clamp(t, -1, 1)
//   v = t * S                  one IEEE multiply, S = 32767 (s16) or 8388607 (s24); never fused with the rounding
//   q = v rounded to the nearest integer, halves away from zero
//
// The rounding is floor-and-compare on |v|: `floor(|v| + 0.5)` is wrong for the double just below 0.5 (the sum rounds up to
// 1), and written as `t * S + 0.5` a compiler that contracts makes one fma of it, which rounds differently at the halves.
#pragma once
#if !defined(__HIPCC_RTC__)
#include <cmath>
#include <cstdint>
#include <cstring>
#endif

#if !defined(DUSP_HOST_DEVICE)
#if defined(__HIPCC__)
#define DUSP_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define DUSP_HOST_DEVICE inline
#endif
#endif

namespace dusp {

constexpr int kPcmS16 = 1, kPcmS24 = 2, kPcmF32 = 3;                 // DUSP_PCM_* of include/dusp_hip.h
constexpr int kNormaliseNone = 0, kNormaliseClip = 1, kNormaliseFull = 2;  // DUSP_NORMALISE_*
constexpr double kPcmScaleS16 = 32767.0, kPcmScaleS24 = 8388607.0;

DUSP_HOST_DEVICE int pcm_bytes_per_sample(int format) { return format == kPcmS16 ? 2 : format == kPcmS24 ? 3 : 4; }

// |x| as an ordered unsigned integer: monotone over the non-NaN values, and every NaN sorts above infinity — the maximum of
// these over an instance IS its peak (bit pattern of an f32), NaN as soon as one sample is.  Order-independent, so exact.
DUSP_HOST_DEVICE uint32_t pcm_abs_bits(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    return b & 0x7fffffffu;
}

// The gain of an instance whose peak has these bits.  CLIP shrinks only what would clip (peak > 1), FULL brings every
// non-silent instance to full scale; a peak that is NaN or infinite (bits >= 0x7f800000) leaves the samples as they are.
DUSP_HOST_DEVICE double pcm_gain(uint32_t peak_bits, int normalise) {
    peak_bits &= 0x7fffffffu;
    if (normalise == kNormaliseNone || peak_bits >= 0x7f800000u) return 1.0;
    if (peak_bits <= (normalise == kNormaliseClip ? 0x3f800000u : 0u)) return 1.0;  // (0x3f800000: 1.0f)
    float peak;
    memcpy(&peak, &peak_bits, 4);
    return 1.0 / (double)peak;
}

DUSP_HOST_DEVICE int32_t pcm_quantise(float x, double g, double scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double t = (double)x * g;
    if (t != t) t = 0.0;
    t = t < -1.0 ? -1.0 : t;
    t = t > 1.0 ? 1.0 : t;
    const double v = t * scale;
    const double a = fabs(v);
    double r = floor(a);
    if (a - r >= 0.5) r += 1.0;  // (a - r is exact)
    const int32_t q = (int32_t)r;
    return v < 0.0 ? -q : q;
}

// format f32: the scaled sample, no clamp, NaN stays
DUSP_HOST_DEVICE float pcm_scale_f32(float x, double g) { return (float)((double)x * g); }

// One sample as the little-endian bytes of its format, in the low bytes of a word (s24: 3 bytes, two's complement).
DUSP_HOST_DEVICE uint32_t pcm_sample_bits(float x, double g, int format) {
    if (format == kPcmF32) {
        const float y = pcm_scale_f32(x, g);
        uint32_t b;
        memcpy(&b, &y, 4);
        return b;
    }
    if (format == kPcmS16) return (uint32_t)pcm_quantise(x, g, kPcmScaleS16) & 0xffffu;
    return (uint32_t)pcm_quantise(x, g, kPcmScaleS24) & 0xffffffu;
}

}  // namespace dusp
