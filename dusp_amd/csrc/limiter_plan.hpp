// limiter_plan.hpp — the host's part of the look-ahead true-peak limiter (limiter_engine.hip has the kernels; dusp_amd/mix.py
// limiter_envelope, limiter_gain, limit, limiter_threshold and check_limiter are the contract): the window's range, how
// a call is cut into workgroups, the threshold a loudness target and a ceiling give, and the words the refusals are made in.
// Plain C++: needs no device.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "truepeak_plan.hpp"

namespace dusp {

constexpr uint32_t kLimiterOne = 1u << 30;        // ONE: the gain curve's fixed point, 30 fractional bits
constexpr uint32_t kLimiterWindowMax = 4096;      // L at the most
constexpr uint32_t kLimiterWindowShort = 512;     // L up to here: the gain kernel with the small halo, a tile of up to 2048 samples
constexpr uint32_t kLimiterPerLaneLong = 4;       // a longer L: a tile of up to 1024 samples, so that two workgroups still fit a CU
constexpr uint32_t kLimiterGroupsPerCu = kTruePeakGroupsPerCu;

constexpr const char *kLimiterNeedsDeliver = "a limiter needs a loudness record with deliver = 1: its threshold is the ceiling seen from the loudness target";
constexpr const char *kLimiterWindowRange = "the limiter's window is 1 .. 4096 samples, not ";
constexpr const char *kLimiterThresholdBad = "the limiter's threshold must be a finite number above 0";

// D: what the interpolator delays by, (K - 1) / 2 — 6 at F = 4, 12 at F = 2, 0 at F = 1
inline uint32_t limiter_delay(uint32_t F) { return (true_peak_phase_taps(F) - 1) / 2; }

// mix.limiter_threshold: the true-peak magnitude the gain of the loudness target brings exactly to the ceiling
inline double limiter_threshold(double lufs, double target_lufs, double ceiling_dbtp) { return std::pow(10.0, ceiling_dbtp / 20.0) / std::pow(10.0, (target_lufs - lufs) / 20.0); }

// How a call over n samples is cut, for BOTH kernels: a workgroup owns W = 256 x per_lane consecutive samples [s0, s0 + W) of the
// timeline — of every row: the rows are looped over inside.  per_lane is the largest of 8, 4, 2, 1 (of 4, 2, 1 where L is above
// kLimiterWindowShort: the gain kernel's two LDS arrays of W + 2 (L - 1) words each must leave room for two workgroups a CU) that still
// gives every CU kLimiterGroupsPerCu workgroups, or 1.
struct LimiterGrid {
    uint32_t per_lane, W;
    uint64_t tiles;
};

inline LimiterGrid limiter_grid(uint64_t n, uint32_t L, int n_cus) {
    const uint64_t want = (uint64_t)(n_cus > 0 ? n_cus : 1) * kLimiterGroupsPerCu;
    LimiterGrid G;
    G.per_lane = L > kLimiterWindowShort ? kLimiterPerLaneLong : kTruePeakPerLaneMax;
    for (;;) {
        G.W = kTruePeakLanes * G.per_lane;
        G.tiles = (n + G.W - 1) / G.W;
        if (G.tiles >= want || G.per_lane == 1) return G;
        G.per_lane /= 2;
    }
}

// reduction from the smallest window sum of a call: min(g), exact
inline double limiter_reduction(uint64_t smallest_sum, uint32_t L) { return (double)smallest_sum / (double)((uint64_t)L * kLimiterOne); }

}  // namespace dusp
