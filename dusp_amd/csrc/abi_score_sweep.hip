// abi_score_sweep.hip — the C ABI (include/dusp_hip.h): the device entries that launch one kernel over flat arrays and have no plan — the
// return of the buses (dusp_score_return_device, dusp_score_stems_return_device), the mix of the tracks (dusp_score_tracks_mix_device,
// dusp_score_stems_mix_device) and the one peak of a block's signals (dusp_peak_common_device).  One check of what they all take, and
// abi_score.hpp's frame of a launch without a plan; the host renders of pieces (abi_piece.hip) launch the same kernels themselves.
#include <cmath>

#include "abi_score.hpp"

struct SweepCount {  // how many buses or tracks a call has, and may have
    size_t n, lo, hi;
    const char *noun;
};

// What a flat sweep is held to, in this order: its counts; null_buffer, the entry's own test of its buffers; 1 .. n_max floats (`need`
// says so); every pointer of `list` — and behind each what each(g) holds entry g to; and the 4-byte alignment of every pointer, `low`
// the entry's own buffers or-ed together
template <class Each>
static int sweep_check(dusp_ctx *ctx, const std::string &w, std::initializer_list<SweepCount> counts, bool null_buffer, size_t n, size_t n_max, const char *need,
                       const float *const *list, size_t n_list, uintptr_t low, Each &&each) {
    for (const SweepCount &c : counts)
        if (c.n < c.lo || c.n > c.hi) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has " + std::to_string(c.lo) + " .. " + std::to_string(c.hi) + " " + c.noun + ", not " + std::to_string(c.n));
    if (null_buffer) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
    if (n < 1 || n > n_max) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + need);
    for (size_t g = 0; g < n_list; g++) {
        if (!list[g]) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
        low |= (uintptr_t)list[g];
        if (int rc = each(g)) return rc;
    }
    if (low & 3) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buffers must be 4-byte aligned");
    return DUSP_OK;
}
static int sweep_item_ok(size_t) { return DUSP_OK; }

// the faders and levels of track g, finite (h_levels: [n_buses][n_tracks])
static int sweep_track_values(dusp_ctx *ctx, const std::string &w, size_t g, const float *h_faders, const float *h_levels, size_t n_buses, size_t n_tracks) {
    if (h_faders && !std::isfinite(h_faders[g])) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the fader of track " + std::to_string(g) + " is not finite");
    for (size_t b = 0; b < n_buses; b++)
        if (!std::isfinite(h_levels[b * n_tracks + g]))
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the level of track " + std::to_string(g) + " into bus " + std::to_string(b) + " is not finite");
    return DUSP_OK;
}

// dusp_score_return_device and, with stems, dusp_score_stems_return_device
static int score_return_entry(dusp_ctx *ctx, const char *who, bool stems, const float *d_dry, const float *const *h_wets, size_t n_buses, size_t n_floats, int raw, float *d_out,
                              float *d_stem_direct, float *d_stem_buses, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    return guarded(ctx->err, who, [&]() -> int {
    if (int rc = sweep_check(ctx, who, {{n_buses, 1, dusp::kScoreBusMax, "buses"}}, !d_dry || !d_out || !h_wets || (stems && !d_stem_buses), n_floats, dusp::kScoreRowMax,
                             "need 1..2^31 floats", h_wets, n_buses, (uintptr_t)d_dry | (uintptr_t)d_out | (uintptr_t)d_stem_direct | (uintptr_t)d_stem_buses, sweep_item_ok))
        return rc;
    float *slots[dusp::kScoreBusMax] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t b = 0; stems && b < n_buses; b++) slots[b] = d_stem_buses + b * n_floats;
    return score_unplanned_call(ctx, stream_, [&](hipStream_t stream) {
        HIP_TRY(ctx, dusp::launch_score_return(d_dry, h_wets, (uint32_t)n_buses, d_out, d_stem_direct, stems ? slots : nullptr, n_floats, raw != 0, stream));
        return DUSP_OK;
    });
    });
}

// dusp_score_tracks_mix_device and, with stems — 0 .. 8 tracks, not 1 .. 8 — dusp_score_stems_mix_device
static int score_mix_entry(dusp_ctx *ctx, const char *who, bool stems, const float *d_direct, const float *const *h_tracks, size_t n_tracks, const float *h_faders, size_t n_buses,
                           const float *h_levels, size_t n_floats, int raw, float *d_out, const float *d_feed_init, float *d_feed_out, float *d_stems, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    if (int rc = sweep_check(ctx, w, {{n_tracks, stems ? 0u : 1u, dusp::kScoreTrackMax, "tracks"}, {n_buses, 0, dusp::kScoreBusMax, "buses"}},
                             !d_direct || !d_out || (stems && !d_stems) || (n_tracks && !h_tracks) || (n_buses && ((n_tracks && !h_levels) || !d_feed_out)), n_floats, dusp::kScoreRowMax,
                             "need 1..2^31 floats", h_tracks, n_tracks,
                             (uintptr_t)d_direct | (uintptr_t)d_out | (uintptr_t)d_stems | (n_buses ? (uintptr_t)d_feed_init | (uintptr_t)d_feed_out : 0),
                             [&](size_t g) { return sweep_track_values(ctx, w, g, h_faders, h_levels, n_buses, n_tracks); }))
        return rc;
    float *slots[dusp::kScoreTrackMax] = {};
    for (size_t g = 0; stems && g < n_tracks; g++) slots[g] = d_stems + (1 + g) * n_floats;
    return score_unplanned_call(ctx, stream_, [&](hipStream_t stream) {
        HIP_TRY(ctx, dusp::launch_score_tracks(d_direct, h_tracks, h_faders, n_buses ? h_levels : nullptr, (uint32_t)n_tracks, (uint32_t)n_buses, d_out, n_buses ? d_feed_init : nullptr,
                                               n_buses ? d_feed_out : nullptr, d_stems, stems ? slots : nullptr, n_floats, raw != 0, stream));
        return DUSP_OK;
    });
    });
}

extern "C" {

// The return of the buses alone: d_out[j] = d_dry[j] + h_wets[0][j] + ... over n_floats floats, left-deep, `|| 0` unless raw
int dusp_score_return_device(dusp_ctx *ctx, const float *d_dry, const float *const *h_wets, size_t n_buses, size_t n_floats, int raw, float *d_out, void *stream_) {
    return score_return_entry(ctx, "dusp_score_return_device", false, d_dry, h_wets, n_buses, n_floats, raw, d_out, nullptr, nullptr, stream_);
}

// ... which keeps the stems: wet b into d_stem_buses + b * n_floats and, d_stem_direct given, d_dry || 0 there
int dusp_score_stems_return_device(dusp_ctx *ctx, const float *d_dry, const float *const *h_wets, size_t n_buses, size_t n_floats, int raw, float *d_out, float *d_stem_direct,
                                   float *d_stem_buses, void *stream_) {
    return score_return_entry(ctx, "dusp_score_stems_return_device", true, d_dry, h_wets, n_buses, n_floats, raw, d_out, d_stem_direct, d_stem_buses, stream_);
}

// The mix of the tracks alone (score_tracks_engine.hip): d_out = d_direct + the tracks' outputs times their faders, left-deep, `|| 0`
// unless raw, and the buses' feeds [n_buses][n_floats] = d_feed_init (NULL: +0) + every term times its level
int dusp_score_tracks_mix_device(dusp_ctx *ctx, const float *d_direct, const float *const *h_tracks, size_t n_tracks, const float *h_faders, size_t n_buses, const float *h_levels,
                                 size_t n_floats, int raw, float *d_out, const float *d_feed_init, float *d_feed_out, void *stream_) {
    return score_mix_entry(ctx, "dusp_score_tracks_mix_device", false, d_direct, h_tracks, n_tracks, h_faders, n_buses, h_levels, n_floats, raw, d_out, d_feed_init, d_feed_out, nullptr,
                           stream_);
}

// ... with 0 .. 8 tracks, which keeps the stems: d_stems [1 + n_tracks][n_floats], slot 0 d_direct || 0 and slot 1 + g term g || 0
int dusp_score_stems_mix_device(dusp_ctx *ctx, const float *d_direct, const float *const *h_tracks, size_t n_tracks, const float *h_faders, size_t n_buses, const float *h_levels,
                                size_t n_floats, int raw, float *d_out, const float *d_feed_init, float *d_feed_out, float *d_stems, void *stream_) {
    return score_mix_entry(ctx, "dusp_score_stems_mix_device", true, d_direct, h_tracks, n_tracks, h_faders, n_buses, h_levels, n_floats, raw, d_out, d_feed_init, d_feed_out, d_stems,
                           stream_);
}

// One peak for n_peaks instances: d_common[i] = the largest of d_peaks, as unsigned words (pcm_engine.hip)
int dusp_peak_common_device(dusp_ctx *ctx, const float *d_peaks, size_t n_peaks, float *d_common, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    const char *who = "dusp_peak_common_device";
    return guarded(ctx->err, who, [&]() -> int {
    if (int rc = sweep_check(ctx, who, {}, !d_peaks || !d_common, n_peaks, (size_t)1 << 24, "need 1..2^24 peaks", nullptr, 0, (uintptr_t)d_peaks | (uintptr_t)d_common, sweep_item_ok)) return rc;
    if (d_peaks == d_common) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": d_common must not be d_peaks: every lane reads all the peaks");
    return score_unplanned_call(ctx, stream_, [&](hipStream_t stream) {
        HIP_TRY(ctx, dusp::launch_pcm_peak_common(d_peaks, d_common, (uint32_t)n_peaks, stream));
        return DUSP_OK;
    });
    });
}

}  // extern "C"
