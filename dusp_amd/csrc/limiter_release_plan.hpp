// limiter_release_plan.hpp — the host's part of the limiter's release (limiter_release_engine.hip has the kernels; dusp_amd/mix.py
// limiter_release_step, limiter_gain_release and check_limiter_release are the contract): the release's range, its
// step, how far back a tile looks for its carry, and what the scratch holds.  Plain C++: needs no device.
#pragma once
#include <cstddef>
#include <cstdint>

#include "limiter_plan.hpp"

namespace dusp {

constexpr uint32_t kLimiterReleaseMax = 1u << 22;  // R at the most, in samples

constexpr const char *kLimiterReleaseRange = "the limiter's release is 1 .. 4194304 samples, not ";

// d = ceil(ONE / R): the most the held curve rises a sample, so a gain of 0 is back at 1 after at most R samples
inline uint32_t limiter_release_step(uint32_t R) { return (kLimiterOne + R - 1) / R; }

// The tiles are limiter_grid's: W = 256 x per_lane positions.  The hold and the release kernel cut j-space, the n + L - 1 positions
// j' = j + (L - 1) of the minima, into hold_tiles of them; the mean / apply kernel cuts the n samples into `tiles`, as the plain apply
// kernel does.  look_back: how many summaries in front of a tile can still reach it — a summary k tiles back comes with d W (k - 1)
// added, which is at least ONE from k - 1 = ceil(ONE / (d W)) on.
struct LimiterReleaseGrid {
    uint32_t per_lane, W, d, look_back;
    uint64_t tiles, hold_tiles, positions;  // positions = n + L - 1
};

inline LimiterReleaseGrid limiter_release_grid(uint64_t n, uint32_t L, uint32_t R, int n_cus) {
    const LimiterGrid G = limiter_grid(n, L, n_cus);
    LimiterReleaseGrid P;
    P.per_lane = G.per_lane, P.W = G.W, P.tiles = G.tiles;
    P.d = limiter_release_step(R);
    P.positions = n + L - 1;
    P.hold_tiles = (P.positions + P.W - 1) / P.W;
    const uint64_t dW = (uint64_t)P.d * P.W;
    P.look_back = (uint32_t)((kLimiterOne + dW - 1) / dW) + 1;
    return P;
}

// the scratch of a call beside the plain limiter's, in 32-bit words: the minima, then the held curve over them in place — one word a
// position — then one summary a hold tile.  The tiles are at least 256 positions wide whatever the device, so this bound holds for any grid
inline uint64_t limiter_release_words(uint64_t n, uint32_t L) { return (n + L - 1) + (n + L - 1 + kTruePeakLanes - 1) / kTruePeakLanes; }

}  // namespace dusp
