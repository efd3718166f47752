// score_stems_engine.hip — the stems of a score or piece (dusp_amd/mix.py stems is the contract): what the mix of the
// tracks and the return of the buses hold for a moment — the direct timeline, every track's term, every bus's output — stored beside the
// mix on the way, each `|| 0`, into slots of n floats of their own; and the one peak the slots and the mix are delivered under.
//
// dusp_score_stems_mix_kernel<B, FADERS>: score_tracks_engine.hip's sweep and arithmetic for the mix and the feeds,
//
//     mix = direct;  feed_b = feed_init ? feed_init[b] : +0                        stem_direct = direct || 0
//     for g in order: term = FADERS ? f32(y_g * f_g) : y_g                         stem_g      = term || 0
//                     mix    = f32(mix + term)
//                     feed_b = f32(feed_b + f32(term * level[b][g]))     for every bus b
//     out = raw ? mix : mix || 0;   feed_out[b] = feed_b  (always raw)
//
// -ffp-contract=off -fno-fast-math, no FMA.  T is a run-time loop over pointers passed BY VALUE, 0 .. 8: with no tracks it is the stem
// and the mix of one timeline.  B (0 .. 4) and FADERS are compile-time, so the 1 + B accumulators are registers and no instantiation
// has a private segment (profiles/score_stems.txt).  Four floats a lane as one 16-byte load and store where every buffer — each feed and
// each slot included — is on a 16-byte boundary, the n % 4 floats behind them one a lane; where any buffer is not, all n floats one a
// lane.  At most kScoreStemsGridMax workgroups of 256 lanes, a lane striding over the items by the launch's lane count.  An item is read
// in full before it is written and no lane touches another's item: out may be direct, feed_out may be feed_init.  A SLOT NEVER ALIASES
// AN INPUT (nor the output).  No LDS, no barrier, no cross-lane operation.
//
// dusp_score_stems_return_kernel: score_send_engine.hip's dusp_score_return_kernel — out = dry; for b: out = f32(out + wet_b); `|| 0`
// unless raw — which also copies every wet_b it reads into the bus's slot, as it is (the bus's copy-out has made it `|| 0`), and, where
// the dry timeline has no slot yet (per-note sends without tracks), dry || 0 into the direct slot.  out may be dry.
//
// dusp_pcm_peak_common_kernel: the n peak words pcm_engine.hip's peak kernel wrote for the block's n instances -> n words, each the
// unsigned maximum of them all, which the encode kernels read as peaks[inst]: one gain for every signal.  One wavefront; every lane reads
// the n words (n is a dozen) and writes its own, so there is nothing to share and no atomic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "score_device.hpp"

namespace dusp {

constexpr uint32_t kScoreStemsGridMax = 2048;  // workgroups of a launch: 256 CUs x 8

struct ScoreStemTracks {  // the tracks' outputs and their slots, each [n] floats, their faders and their levels into the buses; the first n_tracks are used
    const float *p[kScoreTrackMax];
    float *stem[kScoreTrackMax];
    float fader[kScoreTrackMax];
    float level[kScoreBusMax][kScoreTrackMax];
};

// one float or four: the same expressions on each
static __device__ __forceinline__ float score_stems_add(float a, float b) { return a + b; }
static __device__ __forceinline__ float score_stems_mul(float a, float s) { return a * s; }
static __device__ __forceinline__ float score_stems_or0(float a) { return score_or0(a); }
static __device__ __forceinline__ float score_stems_zero(const float *) { return 0.0f; }
static __device__ __forceinline__ float4 score_stems_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
static __device__ __forceinline__ float4 score_stems_mul(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
static __device__ __forceinline__ float4 score_stems_or0(float4 a) { return make_float4(score_or0(a.x), score_or0(a.y), score_or0(a.z), score_or0(a.w)); }
static __device__ __forceinline__ float4 score_stems_zero(const float4 *) { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// item i of every buffer, an item one float (V = float) or four (V = float4): feed b begins n floats behind feed b - 1
template <int B, bool FADERS, class V>
static __device__ __forceinline__ void score_stems_item(const float *direct, const ScoreStemTracks &tracks, uint32_t n_tracks, float *out, const float *feed_init, float *feed_out,
                                                        float *stem_direct, uint64_t n, uint64_t i, int raw) {
    V acc = ((const V *)direct)[i];
    ((V *)stem_direct)[i] = score_stems_or0(acc);
    V feed[B > 0 ? B : 1];
#pragma unroll
    for (int b = 0; b < B; b++) feed[b] = feed_init ? ((const V *)(feed_init + (uint64_t)b * n))[i] : score_stems_zero((const V *)nullptr);
    for (uint32_t g = 0; g < n_tracks; g++) {
        V term = ((const V *)tracks.p[g])[i];
        if (FADERS) term = score_stems_mul(term, tracks.fader[g]);
        ((V *)tracks.stem[g])[i] = score_stems_or0(term);
        acc = score_stems_add(acc, term);
#pragma unroll
        for (int b = 0; b < B; b++) feed[b] = score_stems_add(feed[b], score_stems_mul(term, tracks.level[b][g]));
    }
    ((V *)out)[i] = raw ? acc : score_stems_or0(acc);
#pragma unroll
    for (int b = 0; b < B; b++) ((V *)(feed_out + (uint64_t)b * n))[i] = feed[b];
}

// n_vec items of four floats, then the n - 4 * n_vec floats behind them one an item; `lanes`: the launch's lanes, a lane's stride
template <int B, bool FADERS>
__global__ void __launch_bounds__(256) dusp_score_stems_mix_kernel(const float *direct, ScoreStemTracks tracks, uint32_t n_tracks, float *out, const float *feed_init,
                                                                    float *feed_out, float *stem_direct, uint64_t n, uint64_t n_vec, uint64_t lanes, int raw) {
    const uint64_t items = n_vec + (n - 4 * n_vec);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += lanes) {
        if (i < n_vec)
            score_stems_item<B, FADERS, float4>(direct, tracks, n_tracks, out, feed_init, feed_out, stem_direct, n, i, raw);
        else  // (float 4 * n_vec + (i - n_vec), as a float's index)
            score_stems_item<B, FADERS, float>(direct, tracks, n_tracks, out, feed_init, feed_out, stem_direct, n, 3 * n_vec + i, raw);
    }
}

template <int B>
static void launch_score_stems_mix_b(const float *d_direct, const ScoreStemTracks &tracks, uint32_t n_tracks, bool faders, float *d_out, const float *d_feed_init, float *d_feed_out,
                                     float *d_stem_direct, uint64_t n, uint64_t n_vec, int raw, hipStream_t stream) {
    const uint64_t items = n_vec + (n - 4 * n_vec), groups = (items + 255) / 256;
    const dim3 grid((unsigned)(groups < kScoreStemsGridMax ? groups : kScoreStemsGridMax)), block(256);
    const uint64_t lanes = (uint64_t)grid.x * 256;
    if (faders)
        hipLaunchKernelGGL((dusp_score_stems_mix_kernel<B, true>), grid, block, 0, stream, d_direct, tracks, n_tracks, d_out, d_feed_init, d_feed_out, d_stem_direct, n, n_vec, lanes, raw);
    else
        hipLaunchKernelGGL((dusp_score_stems_mix_kernel<B, false>), grid, block, 0, stream, d_direct, tracks, n_tracks, d_out, d_feed_init, d_feed_out, d_stem_direct, n, n_vec, lanes, raw);
}

// launch_score_tracks (score_tracks_engine.hip) over n floats, 1 <= n <= 2^31, with 0 <= n_tracks <= kScoreTrackMax, which also writes
// d_stem_direct[j] = d_direct[j] || 0 and d_stem_tracks[g][j] = term_g[j] || 0.  The slots are n floats each and alias nothing.
hipError_t launch_score_stems_mix(const float *d_direct, const float *const *d_tracks, const float *h_faders, const float *h_levels, uint32_t n_tracks, uint32_t n_buses,
                                  float *d_out, const float *d_feed_init, float *d_feed_out, float *d_stem_direct, float *const *d_stem_tracks, uint64_t n, int raw,
                                  hipStream_t stream) {
    if (n_tracks > kScoreTrackMax || n_buses > kScoreBusMax) return (hipError_t)1;  // (hipErrorInvalidValue: the callers have checked)
    ScoreStemTracks tracks{};
    uintptr_t low = (uintptr_t)d_direct | (uintptr_t)d_out | (uintptr_t)d_stem_direct;
    for (uint32_t g = 0; g < n_tracks; g++) {
        tracks.p[g] = d_tracks[g];
        tracks.stem[g] = d_stem_tracks[g];
        tracks.fader[g] = h_faders ? h_faders[g] : 1.0f;
        low |= (uintptr_t)d_tracks[g] | (uintptr_t)d_stem_tracks[g];
        for (uint32_t b = 0; b < n_buses; b++) tracks.level[b][g] = h_levels[(size_t)b * n_tracks + g];
    }
    for (uint32_t b = 0; b < n_buses; b++) low |= (uintptr_t)(d_feed_out + (uint64_t)b * n) | (uintptr_t)(d_feed_init ? d_feed_init + (uint64_t)b * n : nullptr);
    const uint64_t n_vec = (low & 15) ? 0 : n / 4;
    const bool faders = h_faders != nullptr && n_tracks > 0;
    switch (n_buses) {
    case 0:
        launch_score_stems_mix_b<0>(d_direct, tracks, n_tracks, faders, d_out, d_feed_init, d_feed_out, d_stem_direct, n, n_vec, raw, stream);
        break;
    case 1:
        launch_score_stems_mix_b<1>(d_direct, tracks, n_tracks, faders, d_out, d_feed_init, d_feed_out, d_stem_direct, n, n_vec, raw, stream);
        break;
    case 2:
        launch_score_stems_mix_b<2>(d_direct, tracks, n_tracks, faders, d_out, d_feed_init, d_feed_out, d_stem_direct, n, n_vec, raw, stream);
        break;
    case 3:
        launch_score_stems_mix_b<3>(d_direct, tracks, n_tracks, faders, d_out, d_feed_init, d_feed_out, d_stem_direct, n, n_vec, raw, stream);
        break;
    default:
        launch_score_stems_mix_b<4>(d_direct, tracks, n_tracks, faders, d_out, d_feed_init, d_feed_out, d_stem_direct, n, n_vec, raw, stream);
        break;
    }
    return hipGetLastError();
}

// ---- the return of the buses, every wet kept ----

struct ScoreStemWets {  // the buses' outputs and their slots, each [n] floats; the first n_buses are used
    const float *p[kScoreBusMax];
    float *stem[kScoreBusMax];
};

// n_vec lanes take four floats each, the n - 4 * n_vec floats behind them one lane each.  stem_direct: nullptr, or where dry || 0 goes
__global__ void __launch_bounds__(256) dusp_score_stems_return_kernel(const float *dry, ScoreStemWets wets, uint32_t n_buses, float *out, float *stem_direct, uint64_t n,
                                                                       uint64_t n_vec, int raw) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_vec) {
        float4 a = ((const float4 *)dry)[i];
        if (stem_direct) ((float4 *)stem_direct)[i] = make_float4(score_or0(a.x), score_or0(a.y), score_or0(a.z), score_or0(a.w));
        for (uint32_t b = 0; b < n_buses; b++) {
            const float4 w = ((const float4 *)wets.p[b])[i];
            ((float4 *)wets.stem[b])[i] = w;
            a.x = a.x + w.x;
            a.y = a.y + w.y;
            a.z = a.z + w.z;
            a.w = a.w + w.w;
        }
        if (!raw) a = make_float4(score_or0(a.x), score_or0(a.y), score_or0(a.z), score_or0(a.w));
        ((float4 *)out)[i] = a;
        return;
    }
    const uint64_t j = 4 * n_vec + (i - n_vec);
    if (j >= n) return;
    float a = dry[j];
    if (stem_direct) stem_direct[j] = score_or0(a);
    for (uint32_t b = 0; b < n_buses; b++) {
        const float w = wets.p[b][j];
        wets.stem[b][j] = w;
        a = a + w;
    }
    out[j] = raw ? a : score_or0(a);
}

// launch_score_return (score_send_engine.hip) over n floats, 1 <= n <= 2^31, n_buses <= kScoreBusMax, which also writes
// d_stem_buses[b][j] = d_wets[b][j] and, d_stem_direct given, d_stem_direct[j] = d_dry[j] || 0.  The slots alias nothing.
hipError_t launch_score_stems_return(const float *d_dry, const float *const *d_wets, uint32_t n_buses, float *d_out, float *d_stem_direct, float *const *d_stem_buses, uint64_t n,
                                     int raw, hipStream_t stream) {
    if (n_buses > kScoreBusMax) return (hipError_t)1;  // (hipErrorInvalidValue: the callers have checked)
    ScoreStemWets wets{};
    uintptr_t low = (uintptr_t)d_dry | (uintptr_t)d_out | (uintptr_t)d_stem_direct;
    for (uint32_t b = 0; b < n_buses; b++) {
        wets.p[b] = d_wets[b];
        wets.stem[b] = d_stem_buses[b];
        low |= (uintptr_t)d_wets[b] | (uintptr_t)d_stem_buses[b];
    }
    const uint64_t n_vec = (low & 15) ? 0 : n / 4, lanes = n_vec + (n - 4 * n_vec);
    const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
    hipLaunchKernelGGL(dusp_score_stems_return_kernel, grid, block, 0, stream, d_dry, wets, n_buses, d_out, d_stem_direct, n, n_vec, raw);
    return hipGetLastError();
}

// ---- one peak for every signal of the block ----

constexpr uint32_t kPeakCommonLanes = 64;  // one wavefront

__global__ void __launch_bounds__(kPeakCommonLanes) dusp_pcm_peak_common_kernel(const uint32_t *peaks, uint32_t *common, uint32_t n) {
    uint32_t m = 0;
    for (uint32_t k = 0; k < n; k++) {  // (wave-uniform addresses: every lane the same n words)
        const uint32_t w = peaks[k];
        m = w > m ? w : m;
    }
    for (uint32_t i = threadIdx.x; i < n; i += kPeakCommonLanes) common[i] = m;
}

// d_common[i] = the unsigned maximum of d_peaks[0 .. n) for every i < n (peak words are `bits & 0x7fffffff`, any NaN above infinity:
// pcm_engine.hip); n >= 1.  d_common is not d_peaks.
hipError_t launch_pcm_peak_common(const float *d_peaks, float *d_common, uint32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(dusp_pcm_peak_common_kernel, dim3(1), dim3(kPeakCommonLanes), 0, stream, (const uint32_t *)d_peaks, (uint32_t *)d_common, n);
    return hipGetLastError();
}

}  // namespace dusp
