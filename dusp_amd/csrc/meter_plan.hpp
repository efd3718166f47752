// meter_plan.hpp — the host's part of the meters (meter_engine.hip has the kernels; dusp_amd/mix.py meters is the contract; DESIGN.md
// 6.18): the K-weighting's coefficients at a sample rate, how a call is cut into segments and what scratch it takes, the segments'
// transition matrix, and what becomes of the hop sums that come down — blocks, the two gates, log10.  Plain C++: needs no device.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

namespace dusp {

constexpr uint32_t kMeterLanes = 256;   // segments a workgroup
constexpr uint32_t kMeterSlice = 32;    // samples of every row in the tile at a time
constexpr uint32_t kMeterSegMax = 512;  // L: the largest divisor of the hop up to this (the hop itself where that is below kMeterSegMin)
constexpr uint32_t kMeterSegMin = 32;    // (at least 2: the combine kernel counts on the input history of M_L being silence)
constexpr uint32_t kMeterBatch = 8;     // segments the combine kernel reads ahead

struct MeterCoef {  // k_weighting's two sections: b0 b1 b2 a1 a2
    double s[2][5];
};
struct MeterMatrix {  // M_L: state after L samples of silence = m * state, the state (x1, x2, y1, y2, z1, z2)
    double m[6][6];
};

// L for a hop: what the kernels, the host and the documents mean by "the segment length"
inline uint32_t meter_segment(uint32_t hop) {
    uint32_t best = 1;
    for (uint32_t d = 1; d <= kMeterSegMax && d <= hop; d++)
        if (hop % d == 0) best = d;
    return best >= kMeterSegMin ? best : hop;
}

constexpr uint32_t kMeterRateMin = 8000;  // the shelf's tan needs sample_rate > 2 x 1682 Hz; the lowest rate the project tests

// 100 ms as a whole number of samples (libebur128's rule); a block is four hops
inline uint32_t meter_hop(uint32_t sample_rate) { return (uint32_t)(((uint64_t)sample_rate + 5) / 10); }
inline size_t meter_blocks(size_t n, uint32_t sample_rate) {
    const size_t hop = meter_hop(sample_rate), block = 4 * hop;
    return !hop || n < block ? 0 : (n - block) / hop + 1;
}

// mix.k_weighting: the shelf and the RLB high-pass by the bilinear re-derivation libebur128 uses, in f64
inline MeterCoef meter_k_weighting(uint32_t sample_rate) {
    const double pi = 3.141592653589793, fs = (double)sample_rate;
    MeterCoef k;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
        k.s[0][0] = (Vh + Vb * K / Q + K * K) / a0;
        k.s[0][1] = 2.0 * (K * K - Vh) / a0;
        k.s[0][2] = (Vh - Vb * K / Q + K * K) / a0;
        k.s[0][3] = 2.0 * (K * K - 1.0) / a0;
        k.s[0][4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / fs), den = 1.0 + K / Q + K * K;
        k.s[1][0] = 1.0;
        k.s[1][1] = -2.0;
        k.s[1][2] = 1.0;
        k.s[1][3] = 2.0 * (K * K - 1.0) / den;
        k.s[1][4] = (1.0 - K / Q + K * K) / den;
    }
    return k;
}

// ---- the host's part of a launch ----

struct MeterGeometry {  // what a call over [rows][n] at `hop` is cut into, and the doubles of scratch it takes
    uint32_t L, per;    // the segment, and the segments of a whole hop
    uint64_t n_seg, n_segs, n_hops;
    uint64_t at_init, at_part, at_hop, doubles;  // scratch: zs [n_segs][6] at 0, init [n_segs][6], part [2][n_segs], per_hop [2][rows][n_hops]
};

inline MeterGeometry meter_geometry(uint64_t rows, uint64_t n, uint32_t hop) {
    MeterGeometry G;
    G.L = meter_segment(hop);
    G.per = hop / G.L;
    G.n_seg = (n + G.L - 1) / G.L;
    G.n_segs = rows * G.n_seg;
    G.n_hops = (n + hop - 1) / hop;
    G.at_init = G.n_segs * 6;
    G.at_part = G.at_init + G.n_segs * 6;
    G.at_hop = G.at_part + 2 * G.n_segs;
    G.doubles = G.at_hop + 2 * rows * G.n_hops;
    return G;
}

// M_L by the recurrence itself, from the six unit states, in f64 on the host
inline void meter_matrix(const MeterCoef &k, uint32_t L, MeterMatrix &M) {
    for (int c = 0; c < 6; c++) {
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        s[c] = 1.0;
        for (uint32_t t = 0; t < L; t++) {
            const double y = k.s[0][1] * s[0] + k.s[0][2] * s[1] - k.s[0][3] * s[2] - k.s[0][4] * s[3];
            const double z = k.s[1][0] * y + k.s[1][1] * s[2] + k.s[1][2] * s[3] - k.s[1][3] * s[4] - k.s[1][4] * s[5];
            s[1] = s[0], s[0] = 0.0, s[3] = s[2], s[2] = y, s[5] = s[4], s[4] = z;
        }
        for (int r = 0; r < 6; r++) M.m[r][c] = s[r];
    }
}


// mix.loudness over one signal: hops f64 [n_hops] the hop sums over its channels, block = 4 hop samples -> momentary [n_blocks] (NULL:
// not asked for) and the gated integrated loudness.  e_j = the four hop sums, added in order, / block.
inline double meter_loudness(const double *hops, size_t n_blocks, size_t block, double *momentary) {
    const double inf = std::numeric_limits<double>::infinity();
    auto energy = [&](size_t j) { return (((hops[j] + hops[j + 1]) + hops[j + 2]) + hops[j + 3]) / (double)block; };
    auto lufs_of = [](double e) { return -0.691 + 10.0 * std::log10(e); };
    bool finite = true;
    for (size_t j = 0; j < n_blocks; j++) {
        const double e = energy(j);
        finite = finite && std::isfinite(e);
        if (momentary) momentary[j] = lufs_of(e);
    }
    if (!finite) return std::numeric_limits<double>::quiet_NaN();
    double sum = 0.0;
    size_t kept = 0;
    for (size_t j = 0; j < n_blocks; j++)
        if (lufs_of(energy(j)) > -70.0) sum += energy(j), kept++;
    if (!kept) return -inf;
    const double gamma = lufs_of(sum / (double)kept) - 10.0;
    sum = 0.0, kept = 0;
    for (size_t j = 0; j < n_blocks; j++) {
        const double l = lufs_of(energy(j));
        if (l > -70.0 && l > gamma) sum += energy(j), kept++;
    }
    return kept ? lufs_of(sum / (double)kept) : -inf;
}

}  // namespace dusp
