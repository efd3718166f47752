// truepeak_plan.hpp — the host's part of the true peak and of a delivery at a loudness target (truepeak_engine.hip has the kernel;
// dusp_amd/mix.py true_peak_taps, true_peak and loudness_gain are the contract): the oversampling factor at a sample
// rate, the windowed-sinc interpolator's taps, how a call is cut into workgroups, and the gain a loudness and a largest true peak
// give.  Plain C++: needs no device.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

namespace dusp {

constexpr uint32_t kTruePeakLanes = 256;      // lanes a workgroup
constexpr uint32_t kTruePeakTaps = 49;        // T: the interpolator's taps, whatever the factor above 1
constexpr uint32_t kTruePeakPerLaneMax = 8;   // output positions a lane at the most: the tile is 256 x (1, 2, 4 or 8) positions
constexpr uint32_t kTruePeakHaloMax = 24;     // K - 1 at the most (F = 2: K = 25)
constexpr uint32_t kTruePeakGroupsPerCu = 4;  // the workgroups a CU should have before a lane takes more positions

struct TruePeakTaps {  // h[j], j = 0 .. 48: phase p owns h[p], h[p + F], ...; passed to the kernel BY VALUE (392 bytes)
    double h[kTruePeakTaps];
};

// F: 4 below 96 kHz, 2 below 192 kHz, else 1 (the true peak is the sample peak)
inline uint32_t true_peak_factor(uint32_t sample_rate) { return sample_rate < 96000 ? 4 : sample_rate < 192000 ? 2 : 1; }
// K: the taps a phase has, a shorter phase padded with a zero tap
inline uint32_t true_peak_phase_taps(uint32_t F) { return F == 1 ? 1 : (kTruePeakTaps + F - 1) / F; }

// mix.true_peak_taps: the Hann-windowed sinc libebur128 interpolates with, in f64; F = 1: h[0] = 1 and nothing else
inline TruePeakTaps true_peak_taps(uint32_t F) {
    const double pi = 3.141592653589793;
    TruePeakTaps t;
    for (uint32_t j = 0; j < kTruePeakTaps; j++) t.h[j] = 0.0;
    if (F == 1) {
        t.h[0] = 1.0;
        return t;
    }
    for (uint32_t j = 0; j < kTruePeakTaps; j++) {
        const int m = (int)j - 24;
        double v = 1.0;
        if (m != 0) {
            const double a = (double)m * pi / (double)F;
            v = m % (int)F == 0 ? 0.0 : std::sin(a) / a;
        }
        t.h[j] = v * (0.5 * (1.0 - std::cos(2.0 * pi * (double)j / 48.0)));
    }
    return t;
}

// How a call over [rows][n] is cut: a workgroup owns W = 256 x per_lane consecutive output positions of ONE row, the row's n + K - 1
// positions (its samples and the filter's tail behind them) take `tiles` workgroups, the last one shorter.  per_lane is the largest of
// 8, 4, 2, 1 that still leaves every CU kTruePeakGroupsPerCu workgroups, or 1: a long call amortises the halo of K - 1 samples a
// tile over 2048 positions, a short one spreads over the chip — and no workgroup is without a position.
struct TruePeakGrid {
    uint32_t per_lane, W;
    uint64_t tiles, groups;
};

inline TruePeakGrid true_peak_grid(uint64_t rows, uint64_t n, uint32_t K, int n_cus) {
    const uint64_t n_out = n + K - 1, want = (uint64_t)(n_cus > 0 ? n_cus : 1) * kTruePeakGroupsPerCu;
    TruePeakGrid G;
    G.per_lane = kTruePeakPerLaneMax;
    for (;;) {
        G.W = kTruePeakLanes * G.per_lane;
        G.tiles = (n_out + G.W - 1) / G.W;
        G.groups = rows * G.tiles;
        if (G.groups >= want || G.per_lane == 1) return G;
        G.per_lane /= 2;
    }
}

// What a word of the kernel says: the bits of |acc| of the largest accumulator, as a double; a NaN where some accumulator was not finite
inline double true_peak_of_word(uint64_t word) {
    double v;
    static_assert(sizeof v == sizeof word, "a word is a double's bits");
    __builtin_memcpy(&v, &word, sizeof v);
    return std::isfinite(v) ? v : std::numeric_limits<double>::quiet_NaN();
}

// mix.loudness_gain: the one gain of a delivery at a loudness target under a true-peak ceiling, as the level word the encoders read —
// the sample magnitude that is brought to full scale — and the gain they then apply, 1 / (double)level.  Unity (1, 1.0f) where the
// loudness is -inf or NaN, where the largest true peak is 0, NaN or Inf, and where the level comes out zero, subnormal or not finite
inline void true_peak_loudness_gain(double lufs, double true_peak_max, double target_lufs, double ceiling_dbtp, double &gain, float &level) {
    gain = 1.0, level = 1.0f;
    if (std::isnan(lufs) || lufs == -std::numeric_limits<double>::infinity()) return;
    if (!(true_peak_max > 0.0) || !std::isfinite(true_peak_max)) return;
    const double by_loudness = std::pow(10.0, (target_lufs - lufs) / 20.0), by_ceiling = std::pow(10.0, ceiling_dbtp / 20.0) / true_peak_max;
    const double G = by_loudness < by_ceiling ? by_loudness : by_ceiling;
    const float l = (float)(1.0 / G);
    if (!std::isnormal(l)) return;
    level = l;
    gain = 1.0 / (double)l;
}

}  // namespace dusp
