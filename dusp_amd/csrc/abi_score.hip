// abi_score.hip — the C ABI (include/dusp_hip.h): voices mixed at per-voice onsets into a timeline (score_plan.hpp and the score engines).
// The plans' image on the device and the one launch path (declared in abi_score.hpp for the other files that launch score kernels), the
// device entries with a plan (dusp_score_device; dusp_score_rows_device and its pan, frac, space, stereo and send forms),
// dusp_score_last_ms, and the host round trip of a score, dusp_render_host_score.  abi_piece.hip has the host renders of pieces,
// abi_score_sweep.hip the device entries without a plan.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "abi_score.hpp"
#include "render_plan.hpp"

// ---- the plans' image ----

int score_image_begin(dusp_ctx *ctx) {
    if (!ctx->score_uploaded) {
        HIP_TRY(ctx, hipEventCreate(&ctx->score_uploaded));  // (with timing: dusp_score_last_ms)
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->score_done, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreate(&ctx->score_up0));
        HIP_TRY(ctx, hipEventCreate(&ctx->score_t0));
        HIP_TRY(ctx, hipEventCreate(&ctx->score_t1));
    } else {
        HIP_TRY(ctx, hipEventSynchronize(ctx->score_uploaded));
    }
    ctx->h_score_plan.clear();
    ctx->score_upload_timed = false;  // (score_up0 .. score_uploaded are about to be another call's)
    return DUSP_OK;
}

// a made plan of n voices: appended to the context's host image on the boundary of its record, and its launch described in L
template <class Record>
static void score_image_add(dusp_ctx *ctx, const dusp::ScorePlanT<Record> &P, size_t n, ScoreLaunch &L) {
    L.w_lo = (uint64_t)P.w_lo;
    L.w_hi = (uint64_t)P.w_hi;
    L.block_shift = P.block_shift;
    L.first_block = P.first_block;
    L.any = P.n_entries() > 0;
    if (L.any) {
        L.n_voices = n;
        L.n_block_first = P.block_first.size();
        L.at = dusp::score_plan_pack(P, ctx->h_score_plan);
    }
}
// one record a voice of the plan just added (L), appended behind it on the boundary of the record: they go up with the plan
template <class Record, class Make>
static size_t score_image_append(dusp_ctx *ctx, size_t n, Make &&make) {
    std::vector<unsigned char> &image = ctx->h_score_plan;
    const size_t at = (image.size() + alignof(Record) - 1) & ~(alignof(Record) - 1);
    image.resize(at + n * sizeof(Record));
    for (size_t k = 0; k < n; k++) {
        const Record r = make(k);
        std::memcpy(image.data() + at + k * sizeof r, &r, sizeof r);
    }
    return at;
}

// plans the voices [0, n) of a contiguous batch within budget_bytes and adds the plan to the image
int score_voices_add(dusp_ctx *ctx, const char *who, const int64_t *h_onsets, const int64_t *h_lengths, size_t n, size_t first_voice, uint64_t n_voice,
                            uint64_t n_total, bool whole_timeline, size_t budget_bytes, ScoreLaunch &L) {
    dusp::ScorePlan P;
    const int64_t bad = dusp::score_plan(h_onsets, h_lengths, n, n_voice, n_total, whole_timeline, budget_bytes, P);
    if (bad >= 0)
        CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the length of voice " + std::to_string(first_voice + (size_t)bad) + " is " + std::to_string(h_lengths[bad]) +
                                        ": lengths must lie in 0 .. n_voice_samples");
    score_image_add(ctx, P, n, L);
    return DUSP_OK;
}

// the pan coefficients of the voices [0, n) of the rows plan just added (L), where the call has pans.  h_comp NULL: the reference's
// compensation by the host's pow (Pan.js:20).  A voice of a stereo call that is not placed (its pan NaN) has zeros, which nobody
// multiplies by
static void score_pans_add(dusp_ctx *ctx, const ScorePlacement &place, size_t n, ScoreLaunch &L) {
    if (!L.any || (place.kind != ScoreKind::pan && place.kind != ScoreKind::stereo)) return;
    L.pan_at = score_image_append<dusp::ScorePan>(ctx, n, [&](size_t k) {
        if (std::isnan(place.h_pans[k])) return dusp::ScorePan{0.0, 0.0, 0.0, 0.0};
        const double comp = place.h_comp ? place.h_comp[k] : std::pow(10.0, ((1.0 - std::fabs((double)place.h_pans[k])) * 1.5) / 20.0);
        return dusp::score_pan_coefficients(place.h_pans[k], comp);
    });
}

// ... and the voices [0, n) that are rows — voice k row_samples[k] samples a channel at device address rows[k].  listed (optional): which
// voices reach the timeline (NULL: nobody asks).  place: these voices' placement, checked.  Where a listed voice has a fraction, the
// voices' weights (dusp::ScoreFrac, 16 bytes a voice on top of the budget) follow the plan and the launch is the two-tap kernel's —
// else the image and the launch are as without.  Behind them the pan coefficients, where the call has pans (score_pans_add).
int score_rows_add(dusp_ctx *ctx, const char *who, const int64_t *h_onsets, const int64_t *h_lengths, const uint32_t *row_samples, const uint64_t *rows, size_t n,
                          size_t first_voice, uint64_t n_total, bool whole_timeline, size_t budget_bytes, const ScorePlacement &place, ScoreLaunch &L,
                          std::vector<unsigned char> *listed, const size_t *voice_ids) {  // (voice_ids: gathered voices' own numbers, for the refusal)
    const bool taps = place.kind == ScoreKind::space;
    const double *h_fracs = place.h_fracs;
    dusp::ScoreRowsPlan P;
    std::vector<dusp::ScoreSpaceTap> T;  // (space: the voices' taps, [voice][speaker], 32 bytes each on top of the budget as the weights are)
    if (taps) {
        T.resize(n * place.n_speakers);
        for (size_t j = 0; j < T.size(); j++) T[j] = dusp::score_space_tap(place.h_delays[j], place.h_tap_gains[j]);
    }
    const dusp::ScorePlacing by{h_fracs, taps ? T.data() : nullptr, place.n_speakers, place.h_row_channels, place.h_pans};  // (row_channels with pans: every voice's kind)
    const int64_t bad = dusp::score_rows_plan(h_onsets, h_lengths, row_samples, rows, n, n_total, whole_timeline, budget_bytes, P, by);
    if (bad >= 0)
        CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the length of voice " + std::to_string(voice_ids ? voice_ids[bad] : first_voice + (size_t)bad) + " is " +
                                        std::to_string(h_lengths[bad]) + ": lengths must lie in 0 .. the voice's own row samples (" + std::to_string(row_samples[bad]) + ")");
    score_image_add(ctx, P, n, L);
    if (taps && L.any) L.space_at = score_image_append<dusp::ScoreSpaceTap>(ctx, T.size(), [&](size_t j) { return T[j]; });
    for (size_t k = 0; k < n && L.any && !L.frac && !taps; k++) L.frac = P.voices[k].hi > P.voices[k].lo && P.voices[k].pad != 0;
    if (L.frac) L.frac_at = score_image_append<dusp::ScoreFrac>(ctx, n, [&](size_t k) { return dusp::score_frac_weights(h_fracs[k]); });
    score_pans_add(ctx, place, n, L);
    L.n_buses = place.n_buses;
    if (L.any && place.n_buses)  // (16 bytes a voice on top of the budget, as the weights are)
        L.send_at = score_image_append<dusp::ScoreSend>(ctx, n, [&](size_t k) {
            dusp::ScoreSend r{{0.0f, 0.0f, 0.0f, 0.0f}};
            for (size_t b = 0; b < place.n_buses; b++) r.level[b] = place.h_sends[b * place.sends_stride + k];
            return r;
        });
    if (listed) {
        listed->resize(n);
        for (size_t k = 0; k < n; k++) (*listed)[k] = P.voices[k].hi > P.voices[k].lo;
    }
    return DUSP_OK;
}

// the image to the device, ordered on `stream` behind the last launch that read the buffer (whatever stream that one ran on)
int score_image_upload(dusp_ctx *ctx, hipStream_t stream) {
    const size_t n_bytes = ctx->h_score_plan.size();
    if (!n_bytes) return DUSP_OK;
    if (n_bytes > ctx->score_plan_cap) {
        if (ctx->d_score_plan) HIP_TRY(ctx, hipFree(ctx->d_score_plan));  // (waits for the device: no launch is reading it any more)
        ctx->d_score_plan = nullptr;
        ctx->score_plan_cap = 0;
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_score_plan, n_bytes + g_guard_bytes));
        if (g_guard_bytes) HIP_TRY(ctx, hipMemset(ctx->d_score_plan + n_bytes, kGuardPattern, g_guard_bytes));
        ctx->score_plan_cap = n_bytes;
    }
    HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->score_done, 0));
    HIP_TRY(ctx, hipEventRecord(ctx->score_up0, stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_score_plan, ctx->h_score_plan.data(), n_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipEventRecord(ctx->score_uploaded, stream));
    return DUSP_OK;
}

// ---- the one launch path ----

// The launch L describes, over its window of a timeline [n_channels][n_total] (pan: mono rows, [2][n_total]).  Its plan is in the image
// on the device (the buffer and L.at: both on 32-byte boundaries); a launch without voices has none and hands the kernel of its kind NULLs.
// d_planar, n_voice: the batch of a contiguous launch (else NULL and 0).  d_send_init, d_send_out: the send timelines
// [L.n_buses][n_channels][n_total] of a rows or pan launch with buses (d_send_out NULL: a launch without).
int score_launch(dusp_ctx *ctx, const ScoreLaunch &L, size_t n_channels, size_t n_total, const float *d_gains, const float *d_init, int raw, float *d_out,
                        hipStream_t stream, const float *d_planar, size_t n_voice, const float *d_send_init, float *d_send_out) {
    if (L.w_hi <= L.w_lo) return DUSP_OK;
    const unsigned char *d_image = ctx->d_score_plan;
    const unsigned char *d_voices = L.any ? d_image + L.at : nullptr;
    const size_t record = L.kind == ScoreKind::contiguous ? sizeof(dusp::ScoreVoice) : sizeof(dusp::ScoreRow);
    const uint32_t *d_block_first = L.any ? (const uint32_t *)(d_voices + L.n_voices * record) : nullptr, *d_entries = L.any ? d_block_first + L.n_block_first : nullptr;
    const dusp::ScoreRow *d_rows = (const dusp::ScoreRow *)d_voices;
    const dusp::ScorePan *d_pans = L.any && (L.kind == ScoreKind::pan || L.kind == ScoreKind::stereo) ? (const dusp::ScorePan *)(d_image + L.pan_at) : nullptr;
    if (d_send_out)  // (score_send_engine.hip: the rows or the pan chain, and every bus's beside it; without voices a copy of both inits)
        HIP_TRY(ctx, dusp::launch_score_send(d_gains, L.any ? (const dusp::ScoreSend *)(d_image + L.send_at) : nullptr, d_pans, d_rows, d_block_first, d_entries, d_init, d_out,
                                             d_send_init, d_send_out, (uint32_t)L.n_buses, (uint32_t)n_channels, n_total, L.w_lo, L.w_hi, L.block_shift, L.first_block, raw,
                                             L.kind == ScoreKind::pan, stream));
    else if (L.any && L.kind == ScoreKind::stereo)  // (score_stereo_engine.hip: rows of one and of two channels into a timeline of two)
        HIP_TRY(ctx, dusp::launch_score_stereo(d_gains, d_pans, L.frac ? (const dusp::ScoreFrac *)(d_image + L.frac_at) : nullptr, d_rows, d_block_first, d_entries, d_init, d_out,
                                               n_total, L.w_lo, L.w_hi, L.block_shift, L.first_block, raw, stream));
    else if (L.any && L.kind == ScoreKind::space)  // (score_space_engine.hip: mono rows into a timeline of n_channels speakers)
        HIP_TRY(ctx, dusp::launch_score_space(d_gains, (const dusp::ScoreSpaceTap *)(d_image + L.space_at), d_rows, d_block_first, d_entries, d_init, d_out, (uint32_t)n_channels,
                                              n_total, L.w_lo, L.w_hi, L.block_shift, L.first_block, raw, stream));
    else if (L.any && L.frac)  // (score_frac_engine.hip: plain rows of n_channels, or — d_pans — panned mono rows)
        HIP_TRY(ctx, dusp::launch_score_frac(d_gains, d_pans, (const dusp::ScoreFrac *)(d_image + L.frac_at), d_rows, d_block_first, d_entries, d_init, d_out,
                                             L.kind == ScoreKind::pan ? 1u : (uint32_t)n_channels, n_total, L.w_lo, L.w_hi, L.block_shift, L.first_block, raw, stream));
    else if (L.kind == ScoreKind::pan || L.kind == ScoreKind::stereo)  // (stereo without voices: `|| 0`, or a copy, of both channels of d_init)
        HIP_TRY(ctx, dusp::launch_score_pan(d_gains, d_pans, d_rows, d_block_first, d_entries, d_init, d_out, n_total, L.w_lo, L.w_hi, L.block_shift, L.first_block, raw, stream));
    else if (L.kind == ScoreKind::rows || L.kind == ScoreKind::space)  // (space without voices: `|| 0`, or a copy, of d_init's channels)
        HIP_TRY(ctx, dusp::launch_score_rows(d_gains, d_rows, d_block_first, d_entries, d_init, d_out, (uint32_t)n_channels, n_total, L.w_lo, L.w_hi, L.block_shift,
                                             L.first_block, raw, stream));
    else
        HIP_TRY(ctx, dusp::launch_score(d_planar, d_gains, (const dusp::ScoreVoice *)d_voices, d_block_first, d_entries, d_init, d_out, (uint32_t)n_channels, n_voice, n_total,
                                        L.w_lo, L.w_hi, L.block_shift, L.first_block, raw, stream));
    if (L.any) HIP_TRY(ctx, hipEventRecord(ctx->score_done, stream));
    return DUSP_OK;
}

// ---- device entries ----

extern "C" {

int dusp_score_device(dusp_ctx *ctx, const float *d_planar, size_t n_instances, size_t n_channels, size_t n_voice_samples, const int64_t *h_onsets,
                      const int64_t *h_lengths, const float *d_gains, size_t n_total_samples, const float *d_init, int raw, float *d_out, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    return guarded(ctx->err, "dusp_score_device", [&]() -> int {
    if (!d_out || (n_instances && (!d_planar || !h_onsets))) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_device: NULL buffer");
    if (!channels_in_range(n_channels) || n_instances > (1u << 24) || !samples_in_range(n_voice_samples) || !samples_in_range(n_total_samples))
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_device: need 1..64 channels, 0..2^24 instances, 1..2^31 samples a voice and 1..2^31 samples of timeline");
    if (n_channels * n_total_samples > dusp::kScoreRowMax)  // (one lane per float of the timeline: the grid, and the kernel's 32-bit sample positions)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_device: channels x timeline samples must not exceed 2^31: score such a piece channel by channel or in windows of the timeline");
    if (n_channels * n_voice_samples > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_device: channels x voice samples must not exceed 2^31");
    if ((((uintptr_t)d_planar | (uintptr_t)d_gains | (uintptr_t)d_init | (uintptr_t)d_out) & 3) != 0)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_device: the buffers must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = stream_of(ctx, stream_);
    ScoreLaunch L(ScoreKind::contiguous, n_total_samples);  // (no voices: `|| 0`, or a copy, of d_init alone)
    return score_device_call(
        ctx, stream, n_instances != 0, L,
        [&]() {
            return score_voices_add(ctx, "dusp_score_device", h_onsets, h_lengths, n_instances, 0, n_voice_samples, n_total_samples, /*whole_timeline=*/true,
                                    score_plan_budget(ctx), L);
        },
        [&]() { return score_launch(ctx, L, n_channels, n_total_samples, d_gains, d_init, raw != 0, d_out, stream, d_planar, n_voice_samples); });
    });
}

// dusp_score_rows_device and its pan, frac, space and stereo forms: rows of n_channels, placed as `place` says (pan, space: rows of one
// channel; stereo: n_channels is 1 and every row has place.h_row_channels[k]), into a timeline of place.timeline_channels(n_channels)
static int score_rows_device(dusp_ctx *ctx, const char *who, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, size_t n_channels, const int64_t *h_onsets,
                             const int64_t *h_lengths, const float *d_gains, const ScorePlacement &place, size_t n_total_samples, const float *d_init, int raw, float *d_out,
                             void *stream_, const float *d_send_init = nullptr, float *d_send_out = nullptr, bool sends = false) {
    if (!ctx) return DUSP_ERR_ARG;
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    if (int rc = place.check_taps(ctx, who, n_voices, n_total_samples)) return rc;  // (first: the timeline's channel count is theirs)
    const size_t n_out_channels = place.timeline_channels(n_channels);
    if (!d_out || (n_voices && (!h_rows || !h_row_samples || !h_onsets))) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
    if (sends) {  // (dusp_score_rows_send_device)
        if (n_voices || place.n_buses < 1 || place.n_buses > dusp::kScoreBusMax) {
            if (int rc = place.check_sends(ctx, who, n_voices)) return rc;
        }
        if (!d_send_out) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
        if ((((uintptr_t)d_send_init | (uintptr_t)d_send_out) & 3) != 0) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buffers must be 4-byte aligned");
    }
    const bool stereo = place.kind == ScoreKind::stereo;
    if (stereo && n_voices > (1u << 24)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": need 0..2^24 voices");
    if (int rc = place.check_kinds(ctx, who, n_voices)) return rc;  // (before the rows' sizes are looked at: they are channels x samples)
    if (!channels_in_range(n_channels) || n_voices > (1u << 24) || !samples_in_range(n_total_samples))
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": need 1..64 channels, 0..2^24 voices and 1..2^31 samples of timeline");
    if (n_out_channels * n_total_samples > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": channels x timeline samples must not exceed 2^31: score such a piece channel by channel or in windows of the timeline");
    if ((((uintptr_t)d_gains | (uintptr_t)d_init | (uintptr_t)d_out) & 3) != 0) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buffers must be 4-byte aligned");
    for (size_t k = 0; k < n_voices; k++) {
        if ((uint64_t)h_row_samples[k] * (stereo ? place.h_row_channels[k] : n_channels) > dusp::kScoreRowMax)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": voice " + std::to_string(k) + ": channels x row samples must not exceed 2^31");
        if (h_row_samples[k] && !h_rows[k]) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the row of voice " + std::to_string(k) + " is NULL");
        if (h_row_samples[k] && ((uintptr_t)h_rows[k] & 3)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the row of voice " + std::to_string(k) + " must be 4-byte aligned");
    }
    if (int rc = place.check_values(ctx, who, n_voices)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = stream_of(ctx, stream_);
    ScoreLaunch L(place.kind, n_total_samples);  // (no voices: `|| 0`, or a copy, of d_init alone)
    L.n_buses = place.n_buses;
    return score_device_call(
        ctx, stream, n_voices != 0, L,
        [&]() {
            static_assert(sizeof(const float *) == sizeof(uint64_t), "rows are handed to the planner as 64-bit addresses");
            return score_rows_add(ctx, who, h_onsets, h_lengths, h_row_samples, (const uint64_t *)h_rows, n_voices, 0, n_total_samples, /*whole_timeline=*/true,
                                  score_plan_budget(ctx), place, L, nullptr);
        },
        [&]() { return score_launch(ctx, L, n_out_channels, n_total_samples, d_gains, d_init, raw != 0, d_out, stream, nullptr, 0, d_send_init, d_send_out); });
    });
}

// ---- what the last device entry took, and the host renders ----

int dusp_score_last_ms(dusp_ctx *ctx, float *kernel_ms, float *plan_ms, float *upload_ms) {
    if (!ctx) return DUSP_ERR_ARG;
    if (!ctx->score_timed) CTX_FAIL(ctx, DUSP_ERR_STATE, "dusp_score_last_ms: no dusp_score_device call has been launched on this context");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->score_t1));
    float k = 0, u = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&k, ctx->score_t0, ctx->score_t1));
    if (ctx->score_upload_timed) HIP_TRY(ctx, hipEventElapsedTime(&u, ctx->score_up0, ctx->score_uploaded));
    if (kernel_ms) *kernel_ms = k;
    if (plan_ms) *plan_ms = (float)ctx->score_plan_ms;
    if (upload_ms) *upload_ms = u;
    return DUSP_OK;
}

int dusp_render_host_score(dusp_program *prog, size_t n_instances, size_t n_voice_samples, size_t n_total_samples, const float *h_params, const float *h_gains,
                           const int64_t *h_onsets, const int64_t *h_lengths, size_t tile_instances, int format, int normalise, void *h_out, float *h_peak) {
    if (!prog) return DUSP_ERR_ARG;
    dusp_ctx *ctx = prog->ctx;
    return guarded(ctx->err, "dusp_render_host_score", [&]() -> int {
    const size_t n_ch = prog->P.out_bufs.size();
    if (!h_onsets) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_render_host_score: h_onsets is NULL");
    if (!samples_in_range(n_total_samples) || n_ch * n_total_samples > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_render_host_score: the timeline must have 1..2^31 samples and channels x timeline samples must not exceed 2^31: render such a piece in windows of the timeline");
    size_t tile = 0;  // (sized over the VOICE's row: the tile holds voices, the timeline is one row beside it)
    if (int rc = tiled_batch_prepare(prog, "dusp_render_host_score", n_instances, n_voice_samples, h_params, h_gains, tile_instances, format, normalise, h_out, &tile))
        return rc;
    // every tile's plan, over the tile's union window, made and uploaded once: the tiles queue up on the stream without the host waiting
    // (the byte budget is the CALL's, shared out over the tiles: a tile whose lists do not fit its share doubles its block.  What no block
    // size takes away is 28 bytes a voice — its record, one list entry, one block_first word — and 40 a tile)
    std::vector<ScoreLaunch> launches((n_instances + tile - 1) / tile, ScoreLaunch(ScoreKind::contiguous));
    const size_t tile_budget = score_plan_budget(ctx) / launches.size();
    if (int rc = score_image_begin(ctx)) return rc;
    const auto t_plan = std::chrono::steady_clock::now();
    for (size_t lo = 0, i = 0; lo < n_instances; lo += tile, i++)
        if (int rc = score_voices_add(ctx, "dusp_render_host_score", h_onsets + lo, h_lengths ? h_lengths + lo : nullptr, std::min(tile, n_instances - lo), lo, n_voice_samples,
                                     n_total_samples, /*whole_timeline=*/false, tile_budget, launches[i]))
            return rc;
    if (ctx->knobs.jit_log >= 2)  // (DUSP_JIT_LOG=2: what the plans cost the host)
        fprintf(stderr, "[dusp host score] %zu plans (tiles of %zu voices) in %.0f us on the host: %zu bytes, blocks of %u samples in the first tile\n", launches.size(), tile,
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_plan).count(), ctx->h_score_plan.size(), 1u << launches[0].block_shift);
    HIP_TRY(ctx, prog->d_mix.ensure(n_ch * n_total_samples));  // the timeline's running sums
    if (int rc = score_image_upload(ctx, ctx->stream)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(prog->d_mix.p, 0, n_ch * n_total_samples * sizeof(float), ctx->stream));
    TiledBatch whole(prog, n_instances, h_params, h_gains, tile);
    for (size_t lo = 0, i = 0; lo < n_instances; lo += tile, i++) {
        if (launches[i].w_hi <= launches[i].w_lo) continue;  // (no voice of the tile reaches the timeline: nothing to render)
        if (int rc = whole.render_tile(lo, std::min(tile, n_instances - lo), n_voice_samples)) return rc;
        if (int rc = score_launch(ctx, launches[i], n_ch, n_total_samples, h_gains ? prog->d_mix_gains.p : nullptr, prog->d_mix.p, /*raw=*/1, prog->d_mix.p, ctx->stream,
                                  prog->d_host_out.p, n_voice_samples))
            return rc;
    }
    // `|| 0` over the whole timeline — a launch without voices — then the delivery, which waits for the stream, and the guard check
    if (int rc = score_launch(ctx, ScoreLaunch(ScoreKind::contiguous, n_total_samples), n_ch, n_total_samples, nullptr, prog->d_mix.p, /*raw=*/0, prog->d_mix.p, ctx->stream, nullptr, 0))
        return rc;
    if (int rc = deliver_host(prog, prog->d_mix.p, nullptr, 1, n_ch, n_total_samples, format, normalise, h_peak, h_out)) return rc;
    whole.staged = false;
    return score_guards(ctx, "dusp_render_host_score", {&prog->d_mix, &prog->d_mix_gains});
    });
}

int dusp_score_rows_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, size_t n_channels, const int64_t *h_onsets,
                           const int64_t *h_lengths, const float *d_gains, size_t n_total_samples, const float *d_init, int raw, float *d_out, void *stream_) {
    return score_rows_device(ctx, "dusp_score_rows_device", h_rows, h_row_samples, n_voices, n_channels, h_onsets, h_lengths, d_gains, ScorePlacement(ScoreKind::rows),
                             n_total_samples, d_init, raw, d_out, stream_);
}

int dusp_score_rows_pan_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, const int64_t *h_onsets, const int64_t *h_lengths,
                               const float *d_gains, const float *h_pans, const double *h_comp, size_t n_total_samples, const float *d_init, int raw, float *d_out,
                               void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    if (n_voices && !h_pans) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_rows_pan_device: h_pans is NULL");
    // (the kind stands without voices too: `|| 0`, or a copy, of both channels of d_init)
    return score_rows_device(ctx, "dusp_score_rows_pan_device", h_rows, h_row_samples, n_voices, 1, h_onsets, h_lengths, d_gains, ScorePlacement(ScoreKind::pan, nullptr, h_pans, h_comp),
                             n_total_samples, d_init, raw, d_out, stream_);
}

int dusp_score_rows_frac_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, size_t n_channels, const int64_t *h_onsets,
                                const double *h_fracs, const int64_t *h_lengths, const float *d_gains, const float *h_pans, const double *h_comp, size_t n_total_samples,
                                const float *d_init, int raw, float *d_out, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    if (h_pans && n_channels != 1) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_rows_frac_device: a panned voice is mono: n_channels must be 1 with h_pans");
    return score_rows_device(ctx, "dusp_score_rows_frac_device", h_rows, h_row_samples, n_voices, n_channels, h_onsets, h_lengths, d_gains,
                             ScorePlacement(h_pans ? ScoreKind::pan : ScoreKind::rows, h_fracs, h_pans, h_comp), n_total_samples, d_init, raw, d_out, stream_);
}

int dusp_score_rows_space_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, size_t n_speakers, const int64_t *h_onsets,
                                 const int64_t *h_lengths, const float *d_gains, const double *h_delays, const double *h_tap_gains, size_t n_total_samples, const float *d_init,
                                 int raw, float *d_out, void *stream_) {
    return score_rows_device(ctx, "dusp_score_rows_space_device", h_rows, h_row_samples, n_voices, 1, h_onsets, h_lengths, d_gains, ScorePlacement(n_speakers, h_delays, h_tap_gains),
                             n_total_samples, d_init, raw, d_out, stream_);
}

int dusp_score_rows_stereo_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, const uint32_t *h_row_channels, size_t n_voices,
                                  const int64_t *h_onsets, const double *h_fracs, const int64_t *h_lengths, const float *d_gains, const float *h_pans, const double *h_comp,
                                  size_t n_total_samples, const float *d_init, int raw, float *d_out, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    if (n_voices && !h_pans) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_rows_stereo_device: h_pans is NULL");
    if (n_voices && !h_row_channels) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_rows_stereo_device: h_row_channels is NULL");
    ScorePlacement place(ScoreKind::stereo, h_fracs, h_pans, h_comp);  // (the kind stands without voices too: `|| 0`, or a copy, of both channels of d_init)
    place.h_row_channels = h_row_channels;
    return score_rows_device(ctx, "dusp_score_rows_stereo_device", h_rows, h_row_samples, n_voices, 1, h_onsets, h_lengths, d_gains, place, n_total_samples, d_init, raw, d_out,
                             stream_);
}

// The send chain alone (score_send_engine.hip): dusp_score_rows_device — h_pans: dusp_score_rows_pan_device, mono rows into two
// channels — whose every term also goes, times the voice's level, to n_buses send timelines
int dusp_score_rows_send_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, size_t n_channels, const int64_t *h_onsets,
                                const int64_t *h_lengths, const float *d_gains, const float *h_pans, const double *h_comp, size_t n_buses, const float *h_sends,
                                size_t n_total_samples, const float *d_init, int raw, float *d_out, const float *d_send_init, float *d_send_out, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    if (h_pans && n_channels != 1) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_rows_send_device: a panned voice is mono: n_channels must be 1 with h_pans");
    ScorePlacement place(h_pans ? ScoreKind::pan : ScoreKind::rows, nullptr, h_pans, h_comp);
    place.n_buses = n_buses;
    place.sends_stride = n_voices;
    place.h_sends = h_sends;
    return score_rows_device(ctx, "dusp_score_rows_send_device", h_rows, h_row_samples, n_voices, n_channels, h_onsets, h_lengths, d_gains, place, n_total_samples, d_init, raw,
                             d_out, stream_, d_send_init, d_send_out, /*sends=*/true);
}

}  // extern "C"
