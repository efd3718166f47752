// score_tracks_engine.hip — the mix of a piece's tracks (dusp_amd/mix.py track_mix is the contract) and, STEMS, the stems
// it holds for a moment (dusp_amd/mix.py stems): the direct timeline and the outputs of T tracks, each read ONCE, become
// the mix and, with buses, the B feeds of the buses — and with STEMS the direct timeline and every track's term are stored on the way:
//
//     mix = direct;  feed_b = feed_init ? feed_init[b] : +0                        STEMS: stem_direct = direct || 0
//     for g in order: term = FADERS ? f32(y_g * f_g) : y_g                         STEMS: stem_g      = term || 0
//                     mix    = f32(mix + term)
//                     feed_b = f32(feed_b + f32(term * level[b][g]))     for every bus b
//     out = raw ? mix : mix || 0;   feed_out[b] = feed_b  (always raw)
//
// -ffp-contract=off -fno-fast-math, no FMA: every product and every add is an f32 operation rounded by itself.  Every track is in every
// bus's chain: a level of 0 is a multiplication by 0 (NaN * 0 poisons the feed, -x * 0 is -0), as in score_send_engine.hip.
//
//   * all buffers are flat arrays of n floats (the timelines' [C][n_total]); the feeds are [B][n], a stem's slot n floats of its own.  The
//     pointers, faders and levels travel BY VALUE in the kernel's arguments (ScoreTracks<STEMS>, as ScoreWets does): T is a run-time loop
//     over them, wave-uniform scalar loads.  T is 1 .. 8 without stems and 0 .. 8 with: no tracks is the stem and the mix of one timeline.
//   * B (0 .. 4), FADERS and STEMS are COMPILE-TIME parameters: the 1 + B accumulators (four floats each on the wide path) are registers,
//     and no instantiation has a private segment (profiles/score_tracks.txt and profiles/score_stems.txt have the register counts of the
//     twenty).  Without STEMS the kernel's arguments hold no stem pointer at all: the record has no slots and the argument list no
//     stem_direct (a parameter pack that is empty), so every argument lies where it lay before there were stems.
//   * four floats a lane as one 16-byte load and store where every buffer (each feed and each slot included) is on a 16-byte boundary, the
//     n % 4 floats behind them one a lane; where any buffer is not, all n floats one a lane.
//   * the grid is a memory-bound sweep's: at most kScoreTracksGridMax workgroups of 256 lanes (eight a CU of 256 CUs), a lane striding
//     over the items by the launch's lane count.  An item is read in full before it is written and no lane touches another's item, so out
//     may be direct and feed_out may be feed_init; nothing is __restrict__-qualified across them.  A SLOT NEVER ALIASES AN INPUT (nor the
//     output).  No LDS, no barrier, no cross-lane operation.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "score_device.hpp"

namespace dusp {

constexpr uint32_t kScoreTracksGridMax = 2048;  // workgroups of a launch: 256 CUs x 8

template <bool STEMS>
struct ScoreTracks {  // the tracks' outputs, each [n] floats, their faders and their levels into the buses; the first n_tracks are read
    const float *p[kScoreTrackMax];
    float fader[kScoreTrackMax];
    float level[kScoreBusMax][kScoreTrackMax];
};
template <>
struct ScoreTracks<true> {  // ... and the tracks' slots, each [n] floats
    const float *p[kScoreTrackMax];
    float *stem[kScoreTrackMax];
    float fader[kScoreTrackMax];
    float level[kScoreBusMax][kScoreTrackMax];
};

// one float or four: the same expressions on each
static __device__ __forceinline__ float score_tracks_add(float a, float b) { return a + b; }
static __device__ __forceinline__ float score_tracks_mul(float a, float s) { return a * s; }
static __device__ __forceinline__ float score_tracks_or0(float a) { return score_or0(a); }
static __device__ __forceinline__ float score_tracks_zero(const float *) { return 0.0f; }
static __device__ __forceinline__ float4 score_tracks_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
static __device__ __forceinline__ float4 score_tracks_mul(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
static __device__ __forceinline__ float4 score_tracks_or0(float4 a) { return make_float4(score_or0(a.x), score_or0(a.y), score_or0(a.z), score_or0(a.w)); }
static __device__ __forceinline__ float4 score_tracks_zero(const float4 *) { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// item i of every buffer, an item one float (V = float) or four (V = float4): feed b begins n floats behind feed b - 1
template <int B, bool FADERS, bool STEMS, class V>
static __device__ __forceinline__ void score_tracks_item(const float *direct, const ScoreTracks<STEMS> &tracks, uint32_t n_tracks, float *out, const float *feed_init, float *feed_out,
                                                         float *stem_direct, uint64_t n, uint64_t i, int raw) {
    V acc = ((const V *)direct)[i];
    if constexpr (STEMS) ((V *)stem_direct)[i] = score_tracks_or0(acc);
    V feed[B > 0 ? B : 1];
#pragma unroll
    for (int b = 0; b < B; b++) feed[b] = feed_init ? ((const V *)(feed_init + (uint64_t)b * n))[i] : score_tracks_zero((const V *)nullptr);
    for (uint32_t g = 0; g < n_tracks; g++) {
        V term = ((const V *)tracks.p[g])[i];
        if (FADERS) term = score_tracks_mul(term, tracks.fader[g]);
        if constexpr (STEMS) ((V *)tracks.stem[g])[i] = score_tracks_or0(term);
        acc = score_tracks_add(acc, term);
#pragma unroll
        for (int b = 0; b < B; b++) feed[b] = score_tracks_add(feed[b], score_tracks_mul(term, tracks.level[b][g]));
    }
    ((V *)out)[i] = raw ? acc : score_tracks_or0(acc);
#pragma unroll
    for (int b = 0; b < B; b++) ((V *)(feed_out + (uint64_t)b * n))[i] = feed[b];
}

// n_vec items of four floats, then the n - 4 * n_vec floats behind them one an item; `lanes`: the launch's lanes, a lane's stride.
// StemDirect: with STEMS one float *, where direct || 0 goes; without, nothing
template <int B, bool FADERS, bool STEMS, class... StemDirect>
__global__ void __launch_bounds__(256) dusp_score_tracks_kernel(const float *direct, ScoreTracks<STEMS> tracks, uint32_t n_tracks, float *out, const float *feed_init,
                                                                 float *feed_out, StemDirect... stem_direct, uint64_t n, uint64_t n_vec, uint64_t lanes, int raw) {
    static_assert(sizeof...(StemDirect) == (STEMS ? 1 : 0), "stem_direct is an argument of the STEMS instances alone");
    const uint64_t items = n_vec + (n - 4 * n_vec);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += lanes) {
        if (i < n_vec)
            score_tracks_item<B, FADERS, STEMS, float4>(direct, tracks, n_tracks, out, feed_init, feed_out, score_stem_direct(stem_direct...), n, i, raw);
        else  // (float 4 * n_vec + (i - n_vec), as a float's index)
            score_tracks_item<B, FADERS, STEMS, float>(direct, tracks, n_tracks, out, feed_init, feed_out, score_stem_direct(stem_direct...), n, 3 * n_vec + i, raw);
    }
}

// the record of a launch filled in, the width of its items, the grid, and the instance picked by n_buses and the faders
template <bool STEMS>
static void launch_score_tracks_as(const float *d_direct, const float *const *d_tracks, const float *h_faders, const float *h_levels, uint32_t n_tracks, uint32_t n_buses, float *d_out,
                                   const float *d_feed_init, float *d_feed_out, float *d_stem_direct, float *const *d_stem_tracks, uint64_t n, int raw, hipStream_t stream) {
    ScoreTracks<STEMS> tracks{};
    uintptr_t low = (uintptr_t)d_direct | (uintptr_t)d_out | (uintptr_t)d_stem_direct;
    for (uint32_t g = 0; g < n_tracks; g++) {
        tracks.p[g] = d_tracks[g];
        tracks.fader[g] = h_faders ? h_faders[g] : 1.0f;
        low |= (uintptr_t)d_tracks[g];
        if constexpr (STEMS) {
            tracks.stem[g] = d_stem_tracks[g];
            low |= (uintptr_t)d_stem_tracks[g];
        }
        for (uint32_t b = 0; b < n_buses; b++) tracks.level[b][g] = h_levels[(size_t)b * n_tracks + g];
    }
    for (uint32_t b = 0; b < n_buses; b++) low |= (uintptr_t)(d_feed_out + (uint64_t)b * n) | (uintptr_t)(d_feed_init ? d_feed_init + (uint64_t)b * n : nullptr);
    const uint64_t n_vec = (low & 15) ? 0 : n / 4, items = n_vec + (n - 4 * n_vec), groups = (items + 255) / 256;
    const dim3 grid((unsigned)(groups < kScoreTracksGridMax ? groups : kScoreTracksGridMax)), block(256);
    const uint64_t lanes = (uint64_t)grid.x * 256;
    auto launch = [&](auto b, auto faders) {
        constexpr int B = decltype(b)::value;
        constexpr bool FADERS = decltype(faders)::value;
        if constexpr (STEMS)
            hipLaunchKernelGGL((dusp_score_tracks_kernel<B, FADERS, true, float *>), grid, block, 0, stream, d_direct, tracks, n_tracks, d_out, d_feed_init, d_feed_out, d_stem_direct, n,
                               n_vec, lanes, raw);
        else
            hipLaunchKernelGGL((dusp_score_tracks_kernel<B, FADERS, false>), grid, block, 0, stream, d_direct, tracks, n_tracks, d_out, d_feed_init, d_feed_out, n, n_vec, lanes, raw);
    };
    auto with_buses = [&](auto b) { h_faders != nullptr && n_tracks > 0 ? launch(b, std::true_type()) : launch(b, std::false_type()); };
    switch (n_buses) {
    case 0: with_buses(std::integral_constant<int, 0>()); break;
    case 1: with_buses(std::integral_constant<int, 1>()); break;
    case 2: with_buses(std::integral_constant<int, 2>()); break;
    case 3: with_buses(std::integral_constant<int, 3>()); break;
    default: with_buses(std::integral_constant<int, 4>()); break;
    }
}

// d_out[j] = d_direct[j] + term_0[j] + ... (left-deep), `|| 0` unless raw, and d_feed_out[b][j] = d_feed_init[b][j] (nullptr: +0) +
// term_0[j] * levels[b][0] + ... over n floats, 1 <= n <= 2^31; term_g = d_tracks[g] times h_faders[g] (nullptr: as it stands).
// n_buses <= kScoreBusMax (0: no feeds); h_levels: [n_buses][n_tracks] on the host.
// d_stem_direct nullptr: 1 <= n_tracks <= kScoreTrackMax, and d_stem_tracks is not looked at.  d_stem_direct given: the launch also writes
// d_stem_direct[j] = d_direct[j] || 0 and d_stem_tracks[g][j] = term_g[j] || 0, and 0 <= n_tracks <= kScoreTrackMax; the slots are n
// floats each and alias nothing.
hipError_t launch_score_tracks(const float *d_direct, const float *const *d_tracks, const float *h_faders, const float *h_levels, uint32_t n_tracks, uint32_t n_buses,
                               float *d_out, const float *d_feed_init, float *d_feed_out, float *d_stem_direct, float *const *d_stem_tracks, uint64_t n, int raw,
                               hipStream_t stream) {
    if ((!d_stem_direct && n_tracks < 1) || n_tracks > kScoreTrackMax || n_buses > kScoreBusMax) return (hipError_t)1;  // (hipErrorInvalidValue: the callers have checked)
    d_stem_direct ? launch_score_tracks_as<true>(d_direct, d_tracks, h_faders, h_levels, n_tracks, n_buses, d_out, d_feed_init, d_feed_out, d_stem_direct, d_stem_tracks, n, raw, stream)
                  : launch_score_tracks_as<false>(d_direct, d_tracks, h_faders, h_levels, n_tracks, n_buses, d_out, d_feed_init, d_feed_out, nullptr, nullptr, n, raw, stream);
    return hipGetLastError();
}

}  // namespace dusp
