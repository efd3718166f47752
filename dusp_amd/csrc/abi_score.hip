// abi_score.hip — the C ABI (include/dusp_hip.h): voices mixed at per-voice onsets into a timeline (score_plan.hpp and the six score
// engines): the plans' image on the device, the placement of a rows call, the one launch path, the device entries (dusp_score_device;
// dusp_score_rows_device and its pan, frac, space and stereo forms) and the host round trips (dusp_render_host_score;
// dusp_render_host_score_parts and its pan, frac, space and stereo forms; dusp_render_host_score_piece, which is all of them and takes
// the master of a piece; dusp_render_host_score_piece_buses, which adds effect sends: per-voice levels into bus circuits, DESIGN.md 6.15,
// with the device entries dusp_score_rows_send_device and dusp_score_return_device; dusp_render_host_score_piece_tracks, which adds
// tracks: sub-mixes of the piece through circuits of their own, DESIGN.md 6.16, with the device entry dusp_score_tracks_mix_device;
// dusp_render_host_score_piece_stems, which delivers the direct mix, every track and every bus return beside the mix, DESIGN.md 6.17,
// with the device entries dusp_score_stems_mix_device, dusp_score_stems_return_device and dusp_peak_common_device;
// dusp_render_host_score_piece_meters, which also meters what it delivers, DESIGN.md 6.18, with the device entry dusp_meter_device —
// abi_meter.hip has the rest of the meters).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "abi_internal.hpp"
#include "render_plan.hpp"

// ---- the plans of a call: an image on the host, uploaded once, and one description per launch ----

// which kernel a launch is: voices of one contiguous batch (score_engine.hip; dusp_amd/mix.py score_chain is the contract), rows of their
// own (score_rows_engine.hip; score_chain_rows), mono rows placed in the stereo field (score_pan_engine.hip; score_chain_rows_panned), or
// mono rows placed in a space, a delay and a gain per speaker (score_space_engine.hip; score_chain_rows_placed), or rows of one and of two
// channels, the mono ones panned or not, into a timeline of two (score_stereo_engine.hip; score_chain_rows_stereo)
enum class ScoreKind { contiguous, rows, pan, space, stereo };

// What places the voices of a rows call: its kind and the host arrays that go with it, one entry a voice, which the caller owns.  An
// entry fills one in (nothing but the kind set: plain rows) and everything between it and the launch takes it by reference.
struct ScoreGathered {  // what a gathered placement points into
    std::vector<double> fracs, comp, delays, tap_gains;
    std::vector<float> pans;
    std::vector<uint32_t> row_channels;
};

struct ScorePlacement {
    ScoreKind kind;                    // what the call is, whether or not it has voices: the entry says it, once
    const double *h_fracs = nullptr;   // rows, pan, stereo: the voices' fractions of a sample (NULL: none)
    const float *h_pans = nullptr;     // pan: a finite pan a voice.  stereo: NaN says "not placed", and a voice of two channels is not
    const double *h_comp = nullptr;    // ... and the compensation (NULL: the reference's, by the host's pow, Pan.js:20)
    size_t n_speakers = 0;             // space: the taps, f64 [voice][speaker] each
    const double *h_delays = nullptr, *h_tap_gains = nullptr;
    const uint32_t *h_row_channels = nullptr;  // stereo: voice k is a row of h_row_channels[k] channels, one or two
    // rows, pan, with buses (score_send_engine.hip): what voice k gives to bus b is h_sends[b * sends_stride + k], finite
    size_t n_buses = 0, sends_stride = 0;
    const float *h_sends = nullptr;
    explicit ScorePlacement(ScoreKind kind_) : kind(kind_) {}
    ScorePlacement(ScoreKind kind_, const double *fracs, const float *pans, const double *comp) : kind(kind_), h_fracs(fracs), h_pans(pans), h_comp(comp) {}
    ScorePlacement(size_t speakers, const double *delays, const double *tap_gains) : kind(ScoreKind::space), n_speakers(speakers), h_delays(delays), h_tap_gains(tap_gains) {}

    size_t timeline_channels(size_t voice_channels) const { return kind == ScoreKind::space ? n_speakers : kind == ScoreKind::rows ? voice_channels : 2; }
    ScorePlacement tile(size_t lo) const {  // the same placement for the voices from `lo` on
        ScorePlacement t = *this;
        if (h_fracs) t.h_fracs += lo;
        if (h_pans) t.h_pans += lo;
        if (h_comp) t.h_comp += lo;
        if (h_delays) t.h_delays += lo * n_speakers;
        if (h_tap_gains) t.h_tap_gains += lo * n_speakers;
        if (h_row_channels) t.h_row_channels += lo;
        if (h_sends) t.h_sends += lo;
        return t;
    }
    // the same placement for the n voices which[0], which[1], ... alone (a track's of a tile), its arrays copied into `into`; a call
    // with tracks has no per-voice levels (h_sends)
    ScorePlacement gather(const size_t *which, size_t n, ScoreGathered &into) const {
        ScorePlacement t = *this;
        auto take = [&](auto &v, const auto *&h, size_t width) {
            if (!h) return;
            v.resize(n * width);
            for (size_t k = 0; k < n; k++)
                for (size_t c = 0; c < width; c++) v[k * width + c] = h[which[k] * width + c];
            h = v.data();
        };
        take(into.fracs, t.h_fracs, 1);
        take(into.pans, t.h_pans, 1);
        take(into.comp, t.h_comp, 1);
        take(into.delays, t.h_delays, n_speakers);
        take(into.tap_gains, t.h_tap_gains, n_speakers);
        take(into.row_channels, t.h_row_channels, 1);
        return t;
    }

    // buses: how many, the levels, and what sends do not go with (fractions, a space, a stereo piece: later changes); n voices
    int check_sends(dusp_ctx *ctx, const char *who, size_t n) const {
        const std::string w(who);
        if (n_buses < 1 || n_buses > dusp::kScoreBusMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has 1 .. 4 buses, not " + std::to_string(n_buses));
        if (!h_sends) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buses' h_sends is NULL: every bus needs a send level a voice");
        if (h_fracs || kind == ScoreKind::space || kind == ScoreKind::stereo)
            CTX_FAIL(ctx, DUSP_ERR_UNSUPPORTED, w + ": sends go with plain rows and with pans at whole-sample onsets: together with fracs, places or stereo they are refused");
        for (size_t b = 0; b < n_buses; b++)
            for (size_t k = 0; k < n; k++)
                if (!std::isfinite(h_sends[b * sends_stride + k]))
                    CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the send level of voice " + std::to_string(k) + " into bus " + std::to_string(b) + " is not finite");
        return DUSP_OK;
    }

    // The checks of n voices, before anything renders; each holds where the kind has nothing of its sort.  The two entry families run
    // them between checks of their own, each in its own order (which refusal a call with several faults gets is behaviour): the device
    // entries taps, kinds, values; the host renders taps, values and — once the parts say how many channels a voice has — kinds.
    // space: the taps at n_speakers speakers over a timeline of n_total samples
    int check_taps(dusp_ctx *ctx, const char *who, size_t n, size_t n_total) const {
        if (kind != ScoreKind::space) return DUSP_OK;
        const std::string w(who);
        if (n_speakers < 1 || n_speakers > dusp::kScoreSpaceChannelsMax)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a Space has 1 .. 8 speakers, not " + std::to_string(n_speakers));
        if (n && (!h_delays || !h_tap_gains)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the taps' delays or gains are NULL");
        if (n_speakers * n_total > dusp::kScoreRowMax)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": speakers x timeline samples must not exceed 2^31: score such a piece speaker by speaker or in windows of the timeline");
        for (size_t k = 0; k < n; k++)
            for (size_t c = 0; c < n_speakers; c++) {
                const double D = h_delays[k * n_speakers + c], G = h_tap_gains[k * n_speakers + c];
                const std::string at = " of voice " + std::to_string(k) + " at speaker " + std::to_string(c);
                if (!std::isfinite(D)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the delay" + at + " is not finite");
                if (D < 0.0 || D > (double)dusp::kScoreSpaceShiftMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the delay" + at + " is outside [0, 2^24] samples");
                if (!std::isfinite(G)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the gain" + at + " is not finite");
            }
        return DUSP_OK;
    }

    // stereo: the kinds of the voices — a row of one or of two channels; a pan that is NaN says "not placed", and a voice of two
    // channels is not placed
    int check_kinds(dusp_ctx *ctx, const char *who, size_t n) const {
        if (kind != ScoreKind::stereo) return DUSP_OK;
        for (size_t k = 0; k < n; k++) {
            const uint32_t channels = h_row_channels[k];
            if (channels != 1 && channels != 2)
                CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": voice " + std::to_string(k) + " has " + std::to_string(channels) + " channels: a voice of a stereo piece has one or two");
            if (std::isinf(h_pans[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the pan of voice " + std::to_string(k) + " is not finite");
            if (channels == 2 && !std::isnan(h_pans[k]))
                CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": voice " + std::to_string(k) + " has two channels and a pan: a two-channel voice is not panned (its pan must be NaN)");
            if (h_comp && !std::isnan(h_pans[k]) && std::isnan(h_comp[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the compensation of voice " + std::to_string(k) + " is NaN");
        }
        return DUSP_OK;
    }

    // pan: the pans and their compensation; then, whatever the kind, the fractions
    int check_values(dusp_ctx *ctx, const char *who, size_t n) const {
        for (size_t k = 0; kind == ScoreKind::pan && k < n; k++) {
            if (!std::isfinite(h_pans[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the pan of voice " + std::to_string(k) + " is not finite");
            if (h_comp && std::isnan(h_comp[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the compensation of voice " + std::to_string(k) + " is NaN");
        }
        for (size_t k = 0; h_fracs && k < n; k++) {
            if (!std::isfinite(h_fracs[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the fraction of voice " + std::to_string(k) + " is not finite");
            if (h_fracs[k] < 0.0 || h_fracs[k] >= 1.0) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the fraction of voice " + std::to_string(k) + " is outside [0, 1)");
        }
        return DUSP_OK;
    }
};

// one launch's plan inside the context's image
struct ScoreLaunch {
    ScoreKind kind;      // a launch without voices (`|| 0`, or a copy, of d_init alone) keeps the kind of its call
    size_t at = 0, n_voices = 0, n_block_first = 0;  // byte offset of the voices; block_first and the entries follow
    uint64_t w_lo = 0, w_hi = 0, first_block = 0;
    uint32_t block_shift = dusp::kScoreGroupShift;
    bool any = false;  // some voice reaches the timeline (else: no plan in the image)
    size_t pan_at = 0;  // a panned launch: byte offset of its voices' coefficients (dusp::ScorePan), behind the plan
    bool frac = false;   // some listed voice starts between samples: the launch is score_frac_engine.hip's, plain rows or panned ...
    size_t frac_at = 0;  // ... and this the byte offset of its voices' weights (dusp::ScoreFrac), behind the plan
    size_t space_at = 0;  // a space launch: byte offset of its voices' taps (dusp::ScoreSpaceTap, [voice][speaker]), behind the plan
    size_t n_buses = 0, send_at = 0;  // a launch with sends (score_send_engine.hip): how many buses, and the byte offset of its voices' levels (dusp::ScoreSend), behind the plan
    explicit ScoreLaunch(ScoreKind kind_, uint64_t n_total = 0) : kind(kind_), w_hi(n_total) {}  // (n_total: over the whole timeline)
};

// before a call rewrites the context's host image: the last upload has read it
static int score_image_begin(dusp_ctx *ctx) {
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

// what the plans of ONE call may take together, on the host and on the device
static size_t score_plan_budget(dusp_ctx *ctx) { return ctx->knobs.score_plan_kb > 0 ? (size_t)ctx->knobs.score_plan_kb << 10 : dusp::kScorePlanBytes; }

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
static int score_voices_add(dusp_ctx *ctx, const char *who, const int64_t *h_onsets, const int64_t *h_lengths, size_t n, size_t first_voice, uint64_t n_voice,
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
static int score_rows_add(dusp_ctx *ctx, const char *who, const int64_t *h_onsets, const int64_t *h_lengths, const uint32_t *row_samples, const uint64_t *rows, size_t n,
                          size_t first_voice, uint64_t n_total, bool whole_timeline, size_t budget_bytes, const ScorePlacement &place, ScoreLaunch &L,
                          std::vector<unsigned char> *listed, const size_t *voice_ids = nullptr) {  // (voice_ids: gathered voices' own numbers, for the refusal)
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
static int score_image_upload(dusp_ctx *ctx, hipStream_t stream) {
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

static bool score_plan_intact(dusp_ctx *ctx) { return !ctx->d_score_plan || !g_guard_bytes || guard_intact(ctx->d_score_plan + ctx->score_plan_cap); }

// ---- the one launch path ----

// The launch L describes, over its window of a timeline [n_channels][n_total] (pan: mono rows, [2][n_total]).  Its plan is in the image
// on the device (the buffer and L.at: both on 32-byte boundaries); a launch without voices has none and hands the kernel of its kind NULLs.
// d_planar, n_voice: the batch of a contiguous launch (else NULL and 0).  d_send_init, d_send_out: the send timelines
// [L.n_buses][n_channels][n_total] of a rows or pan launch with buses (d_send_out NULL: a launch without).
static int score_launch(dusp_ctx *ctx, const ScoreLaunch &L, size_t n_channels, size_t n_total, const float *d_gains, const float *d_init, int raw, float *d_out,
                        hipStream_t stream, const float *d_planar, size_t n_voice, const float *d_send_init = nullptr, float *d_send_out = nullptr) {
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

// What a device entry does once its arguments hold (dusp_score_device, score_rows_device): a fresh image, the call's plan — plan() adds
// it and describes the launch in L; it is not called without voices, and what it takes on the host is score_plan_ms — its upload, and
// launch() between the events score_t0 and score_t1 (dusp_score_last_ms)
template <class Plan, class Launch>
static int score_device_call(dusp_ctx *ctx, hipStream_t stream, bool voices, const ScoreLaunch &L, Plan &&plan, Launch &&launch) {
    if (voices) {
        if (int rc = score_image_begin(ctx)) return rc;
        const auto t_plan = std::chrono::steady_clock::now();
        if (int rc = plan()) return rc;
        ctx->score_plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_plan).count();
        if (int rc = score_image_upload(ctx, stream)) return rc;
    } else {
        if (!ctx->score_t0) {  // (no plan, but the launch is timed like any other)
            if (int rc = score_image_begin(ctx)) return rc;
        }
        ctx->score_plan_ms = 0;
    }
    ctx->score_timed = false;
    ctx->score_upload_timed = L.any;
    HIP_TRY(ctx, hipEventRecord(ctx->score_t0, stream));
    if (int rc = launch()) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->score_t1, stream));
    ctx->score_timed = true;
    return DUSP_OK;
}

// ---- the meters of a delivery (abi_meter.hip) ----

struct ScoreMetered {  // what a call with meters asked for, and the rate its signals are metered at
    const dusp_score_meters *ask;
    uint32_t sample_rate;
};

// deliver_host of a block that no kernel writes any more, [n_signals][n_ch][n_total] — metered on the way where the call has meters: the
// meter kernels run on the context's stream in front of the peak and encode kernels, over the f32 signals in front of the PCM gain, and
// what they leave is gated once the delivery has waited for the stream
static int deliver_metered(dusp_program *prog, const char *who, const ScoreMetered *metered, const float *d_block, size_t n_signals, size_t n_ch, size_t n_total, int format,
                           int normalise, float *h_peaks, void *h_out, bool common_peak) {
    dusp_ctx *ctx = prog->ctx;
    if (metered)
        if (int rc = meter_launch(ctx, d_block, n_signals, n_ch, n_total, metered->sample_rate, ctx->stream)) return rc;
    if (int rc = deliver_host(prog, d_block, nullptr, n_signals, n_ch, n_total, format, normalise, h_peaks, h_out, common_peak)) return rc;
    if (metered)
        if (int rc = meter_finish(ctx, who, n_signals, n_ch, n_total, metered->sample_rate, ctx->stream, metered->ask->h_rms, metered->ask->h_lufs, metered->ask->h_momentary)) return rc;
    return DUSP_OK;
}

// What a host render ends with once its tiles are added to the timeline's running sums (prog->d_mix, [n_ch][n_total]): `|| 0` over the
// whole timeline — a launch of `kind` without voices — the delivery, which waits for the stream, and the guard check
static int score_deliver_host(dusp_program *prog, const char *who, ScoreKind kind, size_t n_ch, size_t n_total, int format, int normalise, float *h_peak, void *h_out,
                              const ScoreMetered *metered = nullptr) {
    dusp_ctx *ctx = prog->ctx;
    if (int rc = score_launch(ctx, ScoreLaunch(kind, n_total), n_ch, n_total, nullptr, prog->d_mix.p, /*raw=*/0, prog->d_mix.p, ctx->stream, nullptr, 0)) return rc;
    if (int rc = deliver_metered(prog, who, metered, prog->d_mix.p, 1, n_ch, n_total, format, normalise, h_peak, h_out, false)) return rc;
    if (g_guard_bytes && (!prog->d_mix.intact() || !prog->d_mix_gains.intact() || !score_plan_intact(ctx)))
        CTX_FAIL(ctx, DUSP_ERR_HIP, std::string(who) + ": the score kernel wrote past the end of a device buffer: guard bytes overwritten");
    return DUSP_OK;
}

// ---- the master of a piece: one mono circuit over every channel of the timeline ----

// What a piece's master is held to before anything renders; n_ch: the timeline's channels, each an instance of the master.  A bus is
// held to the same rules in the same words but for the noun: the = "bus 2", a = "a bus" (a master: "the master", "a master")
static int score_master_check(dusp_ctx *ctx, const std::string &w, const dusp_score_master *master, const dusp_score_part *parts, size_t n_parts, size_t n_ch, size_t n_total,
                              const std::string &the = "the master", const std::string &a = "a master", const std::string &heard = "") {  // (heard: whose timeline it reads, "send " for a bus, "track " for a track program)
    dusp_program *m = master->prog;
    if (!m) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + "'s program is NULL");
    if (m->ctx != ctx) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " was built on another context: it shares the one of the piece's parts");
    for (size_t p = 0; p < n_parts; p++)
        if (parts[p].prog == m)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " is also part " + std::to_string(p) + ": its buffers would be used twice; build it on its own");
    if (m->P.g.n_inputs != 1)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + a + " reads exactly one input stream (the " + heard + "timeline's channel), this program has " + std::to_string(m->P.g.n_inputs));
    if (m->P.out_bufs.size() != 1)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + a + " has one output channel, this program has " + std::to_string(m->P.out_bufs.size()) +
                                        ": it is applied to every channel of the timeline by itself");
    if (m->resumable)
        CTX_FAIL(ctx, DUSP_ERR_UNSUPPORTED, w + ": a resumable program (DUSP_ENGINE_RESUMABLE) is not " + a + ": every call renders it from its initial state");
    if (m->P.g.n_params > 0 && !master->h_params) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " has parameters but its h_params is NULL");
    if (!samples_in_range(n_total) || n_ch * n_total > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " renders channels x timeline samples, which must not exceed 2^31: render such a piece in windows of the timeline without " + a);
    return DUSP_OK;
}

// What the buses of a piece are held to before anything renders: their number and levels (and what sends do not go with), every
// rule of a master per bus, and a bus that is also the master or another bus
static int score_buses_check(dusp_ctx *ctx, const std::string &w, const dusp_score_buses *buses, const ScorePlacement &place, size_t n_voices, const dusp_score_part *parts,
                             size_t n_parts, const dusp_score_master *master, size_t n_ch, size_t n_total, bool voice_levels = true) {
    if (voice_levels) {
        if (int rc = place.check_sends(ctx, w.c_str(), n_voices)) return rc;
    } else if (buses->n_buses < 1 || buses->n_buses > dusp::kScoreBusMax) {  // (a call with tracks: the levels are the tracks', score_tracks_check)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has 1 .. 4 buses, not " + std::to_string(buses->n_buses));
    }
    if (!buses->buses) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buses' programs are NULL");
    for (size_t b = 0; b < buses->n_buses; b++) {
        const std::string the = "bus " + std::to_string(b);
        if (int rc = score_master_check(ctx, w, &buses->buses[b], parts, n_parts, n_ch, n_total, the, "a bus", "send ")) return rc;
        if (master && master->prog == buses->buses[b].prog)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " is also the master: its buffers would be used twice; build it on its own");
        for (size_t q = 0; q < b; q++)
            if (buses->buses[q].prog == buses->buses[b].prog)
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": buses " + std::to_string(q) + " and " + std::to_string(b) + " are the same program: its buffers would be used twice; build it twice");
    }
    return DUSP_OK;
}

// What a host render with buses does between its last tile and its delivery: every bus in turn rendered over its RAW send timeline
// (d_mix_sends [b], [n_ch][n_total]: channel c the one input stream of instance c) from its initial state into its own d_host_out, as a
// master is (`|| 0` at its own copy-out), then ONE return launch that adds the buses' outputs onto the dry sums in d_mix, left-deep:
// raw where a master follows (which reads the sums as they stand), else with the `|| 0` a delivery without buses applies by a launch
// of its own.  rendered: the buses' batches, which stand until the delivery has waited for the stream.
// With stems (d_stem_buses given; score_stems_engine.hip): the same sum into d_out (nullptr: d_mix in place), every bus's output kept in
// its slot, d_stem_buses + b * the timeline, and — d_stem_direct given: per-note sends, whose dry timeline has no slot yet — dry || 0.
static int score_buses_return(dusp_program *prog, const dusp_score_buses *buses, size_t n_ch, size_t n_total, int raw, std::vector<std::unique_ptr<TiledBatch>> &rendered,
                              float *d_out = nullptr, float *d_stem_direct = nullptr, float *d_stem_buses = nullptr) {
    dusp_ctx *ctx = prog->ctx;
    const float *wets[dusp::kScoreBusMax] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t b = 0; b < buses->n_buses; b++) {
        rendered.emplace_back(new TiledBatch(buses->buses[b].prog, n_ch, buses->buses[b].h_params, nullptr, n_ch));  // (one tile: all channels)
        if (int rc = rendered.back()->render_tile(0, n_ch, n_total, prog->d_mix_sends.p + b * n_ch * n_total)) return rc;
        wets[b] = buses->buses[b].prog->d_host_out.p;
    }
    if (d_stem_buses) {
        float *slots[dusp::kScoreBusMax] = {nullptr, nullptr, nullptr, nullptr};
        for (size_t b = 0; b < buses->n_buses; b++) slots[b] = d_stem_buses + b * n_ch * n_total;
        HIP_TRY(ctx, dusp::launch_score_stems_return(prog->d_mix.p, wets, (uint32_t)buses->n_buses, d_out ? d_out : prog->d_mix.p, d_stem_direct, slots, (uint64_t)n_ch * n_total, raw,
                                                     ctx->stream));
        return DUSP_OK;
    }
    HIP_TRY(ctx, dusp::launch_score_return(prog->d_mix.p, wets, (uint32_t)buses->n_buses, prog->d_mix.p, (uint64_t)n_ch * n_total, raw, ctx->stream));
    return DUSP_OK;
}

// ... and what it ends with behind its delivery: the guard bytes of what the send and return kernels wrote, and every bus's own
static int score_buses_guards(dusp_program *prog, const char *who, const dusp_score_buses *buses) {
    dusp_ctx *ctx = prog->ctx;
    if (g_guard_bytes && (!prog->d_mix.intact() || !prog->d_mix_sends.intact() || !prog->d_mix_gains.intact() || !score_plan_intact(ctx)))
        CTX_FAIL(ctx, DUSP_ERR_HIP, std::string(who) + ": the score kernel wrote past the end of a device buffer: guard bytes overwritten");
    for (size_t b = 0; b < buses->n_buses; b++)
        if (int rc = check_guards(buses->buses[b].prog, ctx->stream)) return rc;
    return DUSP_OK;
}

// ---- the tracks of a piece: sub-mixes through circuits of their own (dusp_amd/mix.py track_mix) ----

// What the tracks of a piece are held to before anything renders: their number, where every voice goes, the faders and levels, what
// tracks do not go with, every rule of a master per track program ("track program p"), a program that is used twice, and the tracks
// every program lists.  slot_of[g]: where track g's timeline lies in d_mix_tracks — the tracks of one program adjacent, in the
// program's order, the tracks without a circuit behind them
static int score_tracks_check(dusp_ctx *ctx, const std::string &w, const dusp_score_tracks *tracks, const dusp_score_buses *buses, size_t n_voices, const dusp_score_part *parts,
                              size_t n_parts, const dusp_score_master *master, size_t n_ch, size_t n_total, std::vector<size_t> &slot_of) {
    const size_t T = tracks->n_tracks;
    if (T < 1 || T > dusp::kScoreTrackMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has 1 .. 8 tracks, not " + std::to_string(T));
    if (!tracks->h_track_of) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the tracks' h_track_of is NULL: every voice goes to a track or, with -1, straight to the mix");
    for (size_t k = 0; k < n_voices; k++)
        if (tracks->h_track_of[k] < -1 || tracks->h_track_of[k] >= (int64_t)T)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": voice " + std::to_string(k) + " names track " + std::to_string(tracks->h_track_of[k]) + " of " + std::to_string(T) +
                                            ": track_of holds -1 (straight to the mix) or a track, 0 .. " + std::to_string(T - 1));
    for (size_t g = 0; tracks->h_faders && g < T; g++)
        if (!std::isfinite(tracks->h_faders[g])) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the fader of track " + std::to_string(g) + " is not finite");
    if (tracks->h_track_sends && !buses) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": track_sends without buses: a level is what a track gives to a bus");
    if (buses && !tracks->h_track_sends)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": buses without track_sends: with tracks every bus needs a level a track (track_sends of shape (buses, tracks))");
    if (buses && buses->h_sends)
        CTX_FAIL(ctx, DUSP_ERR_UNSUPPORTED, w + ": sends and tracks do not go together: with tracks the buses are fed by track_sends, a level a track");
    for (size_t b = 0; buses && b < buses->n_buses; b++)
        for (size_t g = 0; g < T; g++)
            if (!std::isfinite(tracks->h_track_sends[b * T + g]))
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the level of track " + std::to_string(g) + " into bus " + std::to_string(b) + " is not finite");
    if (tracks->n_programs > T) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + std::to_string(tracks->n_programs) + " track programs for " + std::to_string(T) + " tracks: a program serves at least one track");
    if (tracks->n_programs && !tracks->programs) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the tracks' programs are NULL");
    slot_of.assign(T, T);
    size_t slot = 0;
    for (size_t p = 0; p < tracks->n_programs; p++) {
        const dusp_score_track_program &tp = tracks->programs[p];
        const std::string the = "track program " + std::to_string(p);
        const dusp_score_master as_master{tp.prog, tp.h_params};
        if (int rc = score_master_check(ctx, w, &as_master, parts, n_parts, n_ch, n_total, the, "a track program", "track ")) return rc;
        if (master && master->prog == tp.prog) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " is also the master: its buffers would be used twice; build it on its own");
        for (size_t b = 0; buses && b < buses->n_buses; b++)
            if (buses->buses[b].prog == tp.prog)
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " is also bus " + std::to_string(b) + ": its buffers would be used twice; build it on its own");
        for (size_t q = 0; q < p; q++)
            if (tracks->programs[q].prog == tp.prog)
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": track programs " + std::to_string(q) + " and " + std::to_string(p) + " are the same program: its buffers would be used twice; build it twice");
        if (tp.n_tracks < 1 || !tp.h_tracks) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " lists no tracks: a track program serves at least one");
        for (size_t j = 0; j < tp.n_tracks; j++) {
            const size_t g = tp.h_tracks[j];
            if (g >= T) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " lists track " + std::to_string(g) + " of " + std::to_string(T));
            if (slot_of[g] != T) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " lists track " + std::to_string(g) + ", which has a circuit already: a track goes through one");
            slot_of[g] = slot++;
        }
        if (tp.n_tracks * n_ch * n_total > dusp::kScoreRowMax)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " renders (tracks x channels) x timeline samples, which must not exceed 2^31: give tracks of one circuit programs of their own, or render such a piece in windows of the timeline");
    }
    for (size_t g = 0; g < T; g++)
        if (slot_of[g] == T) slot_of[g] = slot++;
    return DUSP_OK;
}

// What a host render with tracks does between its last tile and its buses: every track program rendered ONCE over the adjacent RAW
// timelines of its tracks (d_mix_tracks: instance j * n_ch + c hears channel c of its j-th track) from its initial state into its own
// d_host_out, as a master is (`|| 0` at its own copy-out); then ONE launch of the mix kernel: the direct timeline in d_mix and every
// track's output — its program's, or its raw timeline where it has no circuit — times its fader, left-deep into d_mix in place, and
// times its levels into the buses' feeds (d_mix_sends, from +0).  raw: buses or a master follow, which read the sums as they stand.
// With stems (d_stems given; score_stems_engine.hip): the same mix into d_out (nullptr: d_mix in place), direct || 0 kept in slot 0 of
// d_stems and every track's term || 0 in slot 1 + g, a slot the timeline's floats.
static int score_tracks_mix(dusp_program *prog, const dusp_score_tracks *tracks, const dusp_score_buses *buses, const std::vector<size_t> &slot_of, size_t n_ch, size_t n_total,
                            int raw, std::vector<std::unique_ptr<TiledBatch>> &rendered, float *d_out = nullptr, float *d_stems = nullptr) {
    dusp_ctx *ctx = prog->ctx;
    const size_t row = n_ch * n_total;
    const float *y[dusp::kScoreTrackMax] = {};
    for (size_t g = 0; g < tracks->n_tracks; g++) y[g] = prog->d_mix_tracks.p + slot_of[g] * row;
    for (size_t p = 0; p < tracks->n_programs; p++) {
        const dusp_score_track_program &tp = tracks->programs[p];
        const size_t n_inst = tp.n_tracks * n_ch;
        rendered.emplace_back(new TiledBatch(tp.prog, n_inst, tp.h_params, nullptr, n_inst));  // (one tile: every track and channel)
        if (int rc = rendered.back()->render_tile(0, n_inst, n_total, prog->d_mix_tracks.p + slot_of[tp.h_tracks[0]] * row)) return rc;
        for (size_t j = 0; j < tp.n_tracks; j++) y[tp.h_tracks[j]] = tp.prog->d_host_out.p + j * row;
    }
    if (d_stems) {
        float *slots[dusp::kScoreTrackMax] = {};
        for (size_t g = 0; g < tracks->n_tracks; g++) slots[g] = d_stems + (1 + g) * row;
        HIP_TRY(ctx, dusp::launch_score_stems_mix(prog->d_mix.p, y, tracks->h_faders, tracks->h_track_sends, (uint32_t)tracks->n_tracks, buses ? (uint32_t)buses->n_buses : 0u,
                                                  d_out ? d_out : prog->d_mix.p, nullptr, buses ? prog->d_mix_sends.p : nullptr, d_stems, slots, (uint64_t)row, raw, ctx->stream));
        return DUSP_OK;
    }
    HIP_TRY(ctx, dusp::launch_score_tracks(prog->d_mix.p, y, tracks->h_faders, tracks->h_track_sends, (uint32_t)tracks->n_tracks, buses ? (uint32_t)buses->n_buses : 0u, prog->d_mix.p,
                                           nullptr, buses ? prog->d_mix_sends.p : nullptr, (uint64_t)row, raw, ctx->stream));
    return DUSP_OK;
}

// ... and what it ends with behind its delivery: the guard bytes of the track timelines, and every track program's own
static int score_tracks_guards(dusp_program *prog, const char *who, const dusp_score_tracks *tracks) {
    dusp_ctx *ctx = prog->ctx;
    if (g_guard_bytes && (!prog->d_mix.intact() || !prog->d_mix_tracks.intact() || !prog->d_mix_sends.intact() || !prog->d_mix_gains.intact() || !score_plan_intact(ctx)))
        CTX_FAIL(ctx, DUSP_ERR_HIP, std::string(who) + ": the score kernel wrote past the end of a device buffer: guard bytes overwritten");
    for (size_t p = 0; p < tracks->n_programs; p++)
        if (int rc = check_guards(tracks->programs[p].prog, ctx->stream)) return rc;
    return DUSP_OK;
}

// What a host render with a master ends with once its tiles are added to the running sums (prog->d_mix, [n_ch][n_total]): the RAW sums —
// no `|| 0`: a unit behind a Sum hears the Sum's own values — are the master's input block as they stand, channel c the one input stream
// of instance c; its render from its initial state, deciding as a tile of a mix decides (it waits for its compiled kernel), applies
// `|| 0` at its own copy-out; then the delivery from the master's buffer, which waits for the stream, and the guard checks
static int score_master_deliver_host(dusp_program *prog, const char *who, const dusp_score_master *master, size_t n_ch, size_t n_total, int format, int normalise, float *h_peak,
                                     void *h_out, const ScoreMetered *metered = nullptr) {
    dusp_ctx *ctx = prog->ctx;
    dusp_program *m = master->prog;
    {
        TiledBatch channels(m, n_ch, master->h_params, nullptr, n_ch);  // (one tile: all channels; what changes bits is decided as for a mix)
        if (int rc = channels.render_tile(0, n_ch, n_total, prog->d_mix.p)) return rc;
        if (int rc = deliver_metered(prog, who, metered, m->d_host_out.p, 1, n_ch, n_total, format, normalise, h_peak, h_out, false)) return rc;
        channels.staged = false;  // (the delivery has waited for the stream)
    }
    if (g_guard_bytes && (!prog->d_mix.intact() || !prog->d_mix_gains.intact() || !score_plan_intact(ctx)))
        CTX_FAIL(ctx, DUSP_ERR_HIP, std::string(who) + ": the score kernel wrote past the end of a device buffer: guard bytes overwritten");
    if (int rc = check_guards(m, ctx->stream)) return rc;
    return DUSP_OK;
}

// ---- the stems of a piece: the direct mix, every track and bus return beside the mix (dusp_amd/mix.py stems) ----

// What a host render with stems ends with: the block prog->d_stems, [n_signals][n_ch][n_total], holds every stem, written on the way by
// the mix of the tracks and the return of the buses, and — without a master — the mix in its last slot.  With a master the RAW mix is in
// d_mix as ever: the master's render over it (score_master_deliver_host says how) is copied device to device into the last slot.  Then
// ONE delivery of the block as n_signals instances of n_ch channels, under one gain (deliver_host's common_peak), and the guard checks.
static int score_stems_deliver_host(dusp_program *prog, const char *who, const dusp_score_master *master, size_t n_signals, size_t n_ch, size_t n_total, int format, int normalise,
                                    float *h_peaks, void *h_out, const ScoreMetered *metered = nullptr) {
    dusp_ctx *ctx = prog->ctx;
    const size_t timeline = n_ch * n_total;
    std::unique_ptr<TiledBatch> channels;
    if (master) {
        channels.reset(new TiledBatch(master->prog, n_ch, master->h_params, nullptr, n_ch));  // (one tile: all channels)
        if (int rc = channels->render_tile(0, n_ch, n_total, prog->d_mix.p)) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(prog->d_stems.p + (n_signals - 1) * timeline, master->prog->d_host_out.p, timeline * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (int rc = deliver_metered(prog, who, metered, prog->d_stems.p, n_signals, n_ch, n_total, format, normalise, h_peaks, h_out, /*common_peak=*/true)) return rc;
    if (channels) channels->staged = false;  // (the delivery has waited for the stream)
    if (g_guard_bytes && (!prog->d_stems.intact() || !prog->d_host_peak_common.intact() || !prog->d_mix.intact() || !prog->d_mix_gains.intact() || !score_plan_intact(ctx)))
        CTX_FAIL(ctx, DUSP_ERR_HIP, std::string(who) + ": the score kernel wrote past the end of a device buffer: guard bytes overwritten");
    if (master)
        if (int rc = check_guards(master->prog, ctx->stream)) return rc;
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
    if (int rc = score_deliver_host(prog, "dusp_render_host_score", ScoreKind::contiguous, n_ch, n_total_samples, format, normalise, h_peak, h_out)) return rc;
    whole.staged = false;  // (the delivery has waited for the stream)
    return DUSP_OK;
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

// dusp_render_host_score_parts and its pan, frac, space and stereo forms: the parts' voices placed as `given` says (pan, space: mono
// parts; stereo: parts of one and of two output channels, and the voices' channels, given.h_row_channels, are made here from the
// parts') into a timeline of given.timeline_channels(a voice's).  master (optional; dusp_render_host_score_piece): a mono circuit with one
// input stream, rendered over every channel of the raw timeline before the delivery (score_master_deliver_host).  stems (optional;
// dusp_render_host_score_piece_stems): h_out takes 1 + tracks + buses + 1 signals and h_peak as many peaks (score_stems_deliver_host)
static int render_host_score_parts(const char *who, const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                   const int64_t *h_lengths, const float *h_gains, const ScorePlacement &given, size_t n_total_samples, size_t tile_bytes, int format,
                                   int normalise, void *h_out, float *h_peak, const dusp_score_master *master = nullptr, const dusp_score_buses *buses = nullptr,
                                   const dusp_score_tracks *tracks = nullptr, const dusp_score_stems *stems = nullptr, const dusp_score_meters *meters = nullptr) {
    if (!parts || !n_parts || !parts[0].prog) return DUSP_ERR_ARG;
    dusp_program *prog0 = parts[0].prog;  // (its buffers hold what belongs to the piece: the timeline, the gains, the encoded frames)
    dusp_ctx *ctx = prog0->ctx;
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    const size_t n_ch = prog0->P.out_bufs.size();  // (a voice's)
    ScorePlacement place = given;
    if (buses && !tracks) {  // (the levels travel with the placement: a tile's are its voices'; with tracks the levels are the tracks')
        place.n_buses = buses->n_buses;
        place.sends_stride = n_voices;
        place.h_sends = buses->h_sends;
    }
    const bool stereo = place.kind == ScoreKind::stereo, panned = place.kind == ScoreKind::pan, taps = place.kind == ScoreKind::space;
    if (!h_part_of || !h_onsets) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": h_part_of or h_onsets is NULL");
    if (n_voices < 1 || n_voices > (1u << 24)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": need 1..2^24 voices");
    if (int rc = place.check_taps(ctx, who, n_voices, n_total_samples)) return rc;
    const size_t n_out_ch = place.timeline_channels(n_ch);
    size_t n_listed = 0;
    std::vector<size_t> part_ch(n_parts, n_ch);  // (a part's own: they differ in a stereo piece only)
    for (size_t p = 0; p < n_parts; p++) {
        if (!parts[p].prog) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the program of part " + std::to_string(p) + " is NULL");
        if (parts[p].prog->ctx != ctx) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": part " + std::to_string(p) + " was built on another context: all parts of a piece share one");
        part_ch[p] = parts[p].prog->P.out_bufs.size();
        if (stereo && part_ch[p] != 1 && part_ch[p] != 2)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": part " + std::to_string(p) + " has " + std::to_string(part_ch[p]) + " output channels: a voice of a stereo piece has one or two");
        if (panned && parts[p].prog->P.out_bufs.size() != 1)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": part " + std::to_string(p) + " has " + std::to_string(parts[p].prog->P.out_bufs.size()) +
                                            " output channels: a panned voice is mono");
        if (taps && parts[p].prog->P.out_bufs.size() != 1)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": part " + std::to_string(p) + " has " + std::to_string(parts[p].prog->P.out_bufs.size()) +
                                            " output channels: a placed voice is mono");
        if (!stereo && parts[p].prog->P.out_bufs.size() != n_ch)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": part " + std::to_string(p) + " has " + std::to_string(parts[p].prog->P.out_bufs.size()) + " output channels, part 0 has " +
                                            std::to_string(n_ch) + ": all parts of a piece have the same number");
        for (size_t q = 0; q < p; q++)
            if (parts[q].prog == parts[p].prog)
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": parts " + std::to_string(q) + " and " + std::to_string(p) + " are the same program: its tile buffer would be used twice; make them one part or build it twice");
        n_listed += parts[p].n_instances;
    }
    if (master)
        if (int rc = score_master_check(ctx, w, master, parts, n_parts, n_out_ch, n_total_samples)) return rc;
    if (buses)
        if (int rc = score_buses_check(ctx, w, buses, place, n_voices, parts, n_parts, master, n_out_ch, n_total_samples, /*voice_levels=*/!tracks)) return rc;
    std::vector<size_t> slot_of;  // (with tracks: where track g's timeline lies in d_mix_tracks)
    if (tracks)
        if (int rc = score_tracks_check(ctx, w, tracks, buses, n_voices, parts, n_parts, master, n_out_ch, n_total_samples, slot_of)) return rc;
    // (with stems: the direct mix, the tracks, the buses' returns, and the mix last)
    const size_t n_stem_tracks = tracks ? tracks->n_tracks : 0, n_stem_buses = buses ? buses->n_buses : 0, n_signals = 1 + n_stem_tracks + n_stem_buses + 1;
    if (stems && stems->n_signals != n_signals)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the stems' n_signals is " + std::to_string(stems->n_signals) + ", the call delivers " + std::to_string(n_signals) + ": the direct mix, " +
                                        std::to_string(n_stem_tracks) + " tracks, " + std::to_string(n_stem_buses) + " buses and the mix");
    if (stems && !h_out) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": h_out is NULL: a call with stems delivers its " + std::to_string(n_signals) + " signals there");
    // (with meters: every signal of the delivery, at the parts' sample rate)
    const ScoreMetered metered_as{meters, (uint32_t)prog0->P.g.sample_rate}, *metered = meters ? &metered_as : nullptr;
    if (meters) {
        const size_t n_metered = stems ? n_signals : 1, n_blocks = dusp::meter_blocks(n_total_samples, metered_as.sample_rate);
        if (metered_as.sample_rate < dusp::kMeterRateMin)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": meters need a sample rate of at least 8000 Hz, not " + std::to_string(metered_as.sample_rate) + ": the K-weighting's shelf lies at 1682 Hz");
        if (meters->n_signals != n_metered)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the meters' n_signals is " + std::to_string(meters->n_signals) + ", the call delivers " + std::to_string(n_metered) +
                                            (stems ? ": its stems and the mix" : ": the mix"));
        if (meters->n_blocks != n_blocks)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the meters' n_blocks is " + std::to_string(meters->n_blocks) + ", a timeline of " + std::to_string(n_total_samples) + " samples at " +
                                            std::to_string(metered_as.sample_rate) + " Hz has " + std::to_string(n_blocks) + " blocks (dusp_meter_blocks)");
        if (!meters->h_rms) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the meters' h_rms is NULL: every signal's RMS a channel goes there");
        if (!meters->h_lufs) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the meters' h_lufs is NULL: every signal's loudness goes there");
    }
    if (!samples_in_range(n_total_samples) || n_out_ch * n_total_samples > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the timeline must have 1..2^31 samples and channels x timeline samples must not exceed 2^31: render such a piece in windows of the timeline");
    if (stems && n_signals * n_out_ch * n_total_samples > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": signals x channels x timeline samples must not exceed 2^31 with stems (" + std::to_string(n_signals) + " signals): render such a piece in windows of the timeline");
    if (int rc = place.check_values(ctx, who, n_voices)) return rc;
    // voice k of the chain: the next unused instance of part h_part_of[k]
    std::vector<size_t> instance_of(n_voices), used(n_parts, 0);
    for (size_t k = 0; k < n_voices; k++) {
        if (h_part_of[k] >= n_parts) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": voice " + std::to_string(k) + " names part " + std::to_string(h_part_of[k]) + " of " + std::to_string(n_parts));
        instance_of[k] = used[h_part_of[k]]++;
    }
    std::vector<uint32_t> row_channels;  // (a stereo piece: the voices' own)
    if (stereo) {
        row_channels.resize(n_voices);
        for (size_t k = 0; k < n_voices; k++) row_channels[k] = (uint32_t)part_ch[h_part_of[k]];
        place.h_row_channels = row_channels.data();
    }
    if (int rc = place.check_kinds(ctx, who, n_voices)) return rc;
    for (size_t p = 0; p < n_parts; p++)
        if (used[p] != parts[p].n_instances || n_listed != n_voices)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": h_part_of names part " + std::to_string(p) + " " + std::to_string(used[p]) + " times, the part has " +
                                            std::to_string(parts[p].n_instances) + " instances: every instance is one voice of the chain");
    for (size_t p = 0; p < n_parts; p++) {  // (the sizes the tiles are made from; tiled_batch_prepare below refuses the rest, in front of any render)
        if (int rc = check_batch(ctx, who, parts[p].n_instances, parts[p].n_voice_samples)) return rc;
        if (part_ch[p] * parts[p].n_voice_samples > kMixRowMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": channels x voice samples must not exceed 2^31");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the tiles: runs of the chain's voices whose rows together fit tile_bytes
    std::vector<uint64_t> row_bytes(n_voices);
    std::vector<uint32_t> row_samples(n_voices);
    size_t staged = 0, free_bytes = 0, total_bytes = 0;
    for (size_t k = 0; k < n_voices; k++) {
        row_samples[k] = (uint32_t)parts[h_part_of[k]].n_voice_samples;  // (at most 2^31 / channels: tiled_batch_prepare)
        row_bytes[k] = (uint64_t)part_ch[h_part_of[k]] * row_samples[k] * sizeof(float);
    }
    for (size_t p = 0; p < n_parts; p++) staged += parts[p].prog->d_host_out.cap * sizeof(float);
    if (tile_bytes == 0 && ctx->knobs.mix_tile_mb <= 0) HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
    const std::vector<size_t> starts = dusp::piece_tile_starts(row_bytes.data(), n_voices, tile_bytes, ctx->knobs.mix_tile_mb, free_bytes, staged, ctx->n_cus);
    const size_t n_tiles = starts.size() - 1;
    // a part's share of tile i: its instances [share[p][i], share[p][i + 1]), one contiguous range since its instances enter the chain in
    // their own order; its tile buffer holds the largest share
    std::vector<std::vector<size_t>> share(n_parts, std::vector<size_t>(n_tiles + 1, 0));
    {
        std::vector<size_t> seen(n_parts, 0);
        for (size_t i = 0; i < n_tiles; i++) {
            for (size_t k = starts[i]; k < starts[i + 1]; k++) seen[h_part_of[k]]++;
            for (size_t p = 0; p < n_parts; p++) share[p][i + 1] = seen[p];
        }
    }
    for (size_t p = 0; p < n_parts; p++) {
        size_t most = 1, unused = 0;
        for (size_t i = 0; i < n_tiles; i++) most = std::max(most, share[p][i + 1] - share[p][i]);
        if (int rc = tiled_batch_prepare(parts[p].prog, who, parts[p].n_instances, parts[p].n_voice_samples, parts[p].h_params, nullptr, most, format, normalise, h_out, &unused)) return rc;
    }
    // every tile's plan, over the tile's union window, made up front under the call's one budget and uploaded once: the rows' addresses
    // are known, since the tile buffers stand.  With tracks a tile has one plan a DESTINATION that has voices in it — the direct
    // timeline (0) and every track's (1 + g) — over that destination's voices alone, gathered; tiles ascend, so every destination's
    // chain is in index order.  first_launch[i] .. first_launch[i + 1]: tile i's launches
    struct TileLaunch {
        ScoreLaunch L;
        size_t dest, gains_at;  // which timeline; where its voices' gains begin in d_mix_gains
    };
    std::vector<TileLaunch> launches;
    std::vector<size_t> first_launch(n_tiles + 1, 0);
    std::vector<std::vector<size_t>> members;  // (with tracks: the voices of every launch, by their numbers in the call)
    if (tracks)
        for (size_t i = 0; i < n_tiles; i++) {
            for (size_t dest = 0; dest <= tracks->n_tracks; dest++) {
                std::vector<size_t> which;
                for (size_t k = starts[i]; k < starts[i + 1]; k++)
                    if ((size_t)(tracks->h_track_of[k] + 1) == dest) which.push_back(k);
                if (which.empty()) continue;
                launches.push_back(TileLaunch{ScoreLaunch(place.kind), dest, 0});
                members.push_back(std::move(which));
            }
            first_launch[i + 1] = launches.size();
        }
    else
        for (size_t i = 0; i < n_tiles; i++) {
            launches.push_back(TileLaunch{ScoreLaunch(place.kind), 0, starts[i]});
            first_launch[i + 1] = launches.size();
        }
    std::vector<std::vector<unsigned char>> renders(n_tiles, std::vector<unsigned char>(n_parts, 0));  // does part p render in tile i?
    std::vector<float> ordered_gains;  // (with tracks: the gains in launch order, uploaded once)
    // (the call's one budget, shared out over the tiles; with tracks a tile's share is shared out over its launches by their voices)
    const size_t tile_budget = score_plan_budget(ctx) / n_tiles;
    if (int rc = score_image_begin(ctx)) return rc;
    const auto t_plan = std::chrono::steady_clock::now();
    {
        std::vector<uint64_t> rows;
        std::vector<unsigned char> listed;
        auto row_of = [&](size_t i, size_t k) {  // voice k, of tile i, in its part's tile buffer
            const size_t p = h_part_of[k];
            return (uint64_t)(uintptr_t)(parts[p].prog->d_host_out.p + (instance_of[k] - share[p][i]) * part_ch[p] * parts[p].n_voice_samples);
        };
        for (size_t i = 0; i < n_tiles && !tracks; i++) {
            const size_t lo = starts[i], n = starts[i + 1] - lo;
            rows.resize(n);
            for (size_t k = 0; k < n; k++) rows[k] = row_of(i, lo + k);
            if (int rc = score_rows_add(ctx, who, h_onsets + lo, h_lengths ? h_lengths + lo : nullptr, row_samples.data() + lo, rows.data(), n, lo, n_total_samples,
                                        /*whole_timeline=*/false, tile_budget, place.tile(lo), launches[i].L, &listed))
                return rc;
            for (size_t k = 0; k < n; k++)
                if (listed[k]) renders[i][h_part_of[lo + k]] = 1;
        }
        std::vector<int64_t> onsets, lengths;
        std::vector<uint32_t> samples;
        ScoreGathered gathered;
        for (size_t i = 0; i < n_tiles && tracks; i++)
            for (size_t j = first_launch[i]; j < first_launch[i + 1]; j++) {
                const std::vector<size_t> &which = members[j];
                const size_t n = which.size();
                rows.resize(n);
                onsets.resize(n);
                lengths.resize(n);
                samples.resize(n);
                launches[j].gains_at = ordered_gains.size();
                for (size_t k = 0; k < n; k++) {
                    rows[k] = row_of(i, which[k]);
                    onsets[k] = h_onsets[which[k]];
                    if (h_lengths) lengths[k] = h_lengths[which[k]];
                    samples[k] = row_samples[which[k]];
                    if (h_gains) ordered_gains.push_back(h_gains[which[k]]);
                }
                if (int rc = score_rows_add(ctx, who, onsets.data(), h_lengths ? lengths.data() : nullptr, samples.data(), rows.data(), n, 0, n_total_samples,
                                            /*whole_timeline=*/false, tile_budget * n / (starts[i + 1] - starts[i]), place.gather(which.data(), n, gathered), launches[j].L, &listed,
                                            which.data()))
                    return rc;
                for (size_t k = 0; k < n; k++)
                    if (listed[k]) renders[i][h_part_of[which[k]]] = 1;
            }
    }
    if (ctx->knobs.jit_log >= 2)  // (DUSP_JIT_LOG=2: what the plans cost the host)
        fprintf(stderr, "[dusp host piece] %zu plans over %zu voices of %zu parts in %.0f us on the host: %zu bytes\n", launches.size(), n_voices, n_parts,
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_plan).count(), ctx->h_score_plan.size());
    const size_t timeline = n_out_ch * n_total_samples;
    HIP_TRY(ctx, prog0->d_mix.ensure(timeline));  // the timeline's running sums
    if (master) {  // (... and what the master makes of them: one more [channels][n_total], and its columns)
        HIP_TRY(ctx, master->prog->d_host_out.ensure(timeline));
        if (master->prog->P.g.n_params) HIP_TRY(ctx, master->prog->d_host_par.ensure((size_t)master->prog->P.g.n_params * n_out_ch));
    }
    if (buses) {  // (... the send timelines, and what every bus makes of its own: 2 x n_buses more [channels][n_total], and the buses' columns)
        HIP_TRY(ctx, prog0->d_mix_sends.ensure(buses->n_buses * timeline));
        for (size_t b = 0; b < buses->n_buses; b++) {
            dusp_program *bus = buses->buses[b].prog;
            HIP_TRY(ctx, bus->d_host_out.ensure(timeline));
            if (bus->P.g.n_params) HIP_TRY(ctx, bus->d_host_par.ensure((size_t)bus->P.g.n_params * n_out_ch));
        }
    }
    if (tracks) {  // (... the tracks' timelines, and what every track program makes of its own: one [channels][n_total] a track each, and its columns)
        HIP_TRY(ctx, prog0->d_mix_tracks.ensure(tracks->n_tracks * timeline));
        for (size_t p = 0; p < tracks->n_programs; p++) {
            const dusp_score_track_program &tp = tracks->programs[p];
            HIP_TRY(ctx, tp.prog->d_host_out.ensure(tp.n_tracks * timeline));
            if (tp.prog->P.g.n_params) HIP_TRY(ctx, tp.prog->d_host_par.ensure((size_t)tp.prog->P.g.n_params * tp.n_tracks * n_out_ch));
        }
    }
    if (stems) HIP_TRY(ctx, prog0->d_stems.ensure(n_signals * timeline));  // (... and with stems every signal of the delivery: one more [channels][n_total] each)
    if (h_gains) {  // (4 bytes a voice, where the plans take 32 and more: the whole piece's at once; with tracks in launch order)
        HIP_TRY(ctx, prog0->d_mix_gains.ensure(n_voices));
        HIP_TRY(ctx, hipMemcpyAsync(prog0->d_mix_gains.p, tracks ? ordered_gains.data() : h_gains, n_voices * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    if (int rc = score_image_upload(ctx, ctx->stream)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(prog0->d_mix.p, 0, timeline * sizeof(float), ctx->stream));
    float *d_sends = buses && !tracks ? prog0->d_mix_sends.p : nullptr;  // (with tracks the mix kernel writes the buses' feeds, from +0)
    if (d_sends) HIP_TRY(ctx, hipMemsetAsync(d_sends, 0, buses->n_buses * timeline * sizeof(float), ctx->stream));
    if (tracks) HIP_TRY(ctx, hipMemsetAsync(prog0->d_mix_tracks.p, 0, tracks->n_tracks * timeline * sizeof(float), ctx->stream));
    std::vector<std::unique_ptr<TiledBatch>> whole;  // what changes bits is decided from the WHOLE part
    for (size_t p = 0; p < n_parts; p++) whole.emplace_back(new TiledBatch(parts[p].prog, parts[p].n_instances, parts[p].h_params, share[p]));
    auto waited = [&]() {
        for (auto &b : whole) b->staged = false;
    };
    for (size_t i = 0; i < n_tiles; i++) {
        for (size_t p = 0; p < n_parts; p++)  // (no voice of the tile reaches a timeline: nothing to render)
            if (renders[i][p])
                if (int rc = whole[p]->render_tile(share[p][i], share[p][i + 1] - share[p][i], parts[p].n_voice_samples)) return rc;
        for (size_t j = first_launch[i]; j < first_launch[i + 1]; j++) {
            if (launches[j].L.w_hi <= launches[j].L.w_lo) continue;
            const float *d_gains = h_gains ? prog0->d_mix_gains.p + launches[j].gains_at : nullptr;
            float *d_into = launches[j].dest ? prog0->d_mix_tracks.p + slot_of[launches[j].dest - 1] * timeline : prog0->d_mix.p;  // (in place and raw)
            if (int rc = score_launch(ctx, launches[j].L, n_out_ch, n_total_samples, d_gains, d_into, /*raw=*/1, d_into, ctx->stream, nullptr, 0, d_sends, d_sends)) return rc;
        }
    }
    std::vector<std::unique_ptr<TiledBatch>> tracked, returned;  // (the track programs' renders, and the buses')
    // (with stems: the kernel that makes the mix last keeps the stems on the way, and without a master it writes the mix into the last
    // slot itself; with a master the raw mix stays in d_mix for it.  slot s: d_stems + s timelines)
    float *d_slots = stems ? prog0->d_stems.p : nullptr, *d_last = stems && !master ? d_slots + (n_signals - 1) * timeline : nullptr;
    if (tracks)  // (raw where buses or a master follow; else the mix kernel applies the `|| 0` of the delivery)
        if (int rc = score_tracks_mix(prog0, tracks, buses, slot_of, n_out_ch, n_total_samples, /*raw=*/buses != nullptr || master != nullptr, tracked, buses ? nullptr : d_last, d_slots))
            return rc;
    if (buses)  // (per-note sends: the dry timeline gets its slot here)
        if (int rc = score_buses_return(prog0, buses, n_out_ch, n_total_samples, /*raw=*/master != nullptr, returned, d_last, stems && !tracks ? d_slots : nullptr,
                                        stems ? d_slots + (1 + n_stem_tracks) * timeline : nullptr))
            return rc;
    if (stems && !tracks && !buses)  // (one timeline: its stem and — `|| 0`, as a delivery without stems applies it — the mix; raw and in place in front of a master)
        HIP_TRY(ctx, dusp::launch_score_stems_mix(prog0->d_mix.p, nullptr, nullptr, nullptr, 0, 0, d_last ? d_last : prog0->d_mix.p, nullptr, nullptr, d_slots, nullptr, (uint64_t)timeline,
                                                  /*raw=*/master != nullptr, ctx->stream));
    // (`|| 0` is the rows kernel's over the timeline's channels, panned or not; behind a master it is the master's own copy-out's; behind
    // buses without a master the return kernel has applied it, behind tracks without either the mix kernel)
    if (int rc = stems             ? score_stems_deliver_host(prog0, who, master, n_signals, n_out_ch, n_total_samples, format, normalise, h_peak, h_out, metered)
                 : master          ? score_master_deliver_host(prog0, who, master, n_out_ch, n_total_samples, format, normalise, h_peak, h_out, metered)
                 : buses || tracks ? deliver_metered(prog0, who, metered, prog0->d_mix.p, 1, n_out_ch, n_total_samples, format, normalise, h_peak, h_out, false)
                                   : score_deliver_host(prog0, who, ScoreKind::rows, n_out_ch, n_total_samples, format, normalise, h_peak, h_out, metered))
        return rc;
    waited();  // (the delivery has waited for the stream)
    for (auto &b : returned) b->staged = false;
    for (auto &b : tracked) b->staged = false;
    if (buses)
        if (int rc = score_buses_guards(prog0, who, buses)) return rc;
    if (tracks)
        if (int rc = score_tracks_guards(prog0, who, tracks)) return rc;
    return DUSP_OK;
    });
}

int dusp_render_host_score_parts(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                 const int64_t *h_lengths, const float *h_gains, size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out,
                                 float *h_peak) {
    return render_host_score_parts("dusp_render_host_score_parts", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, ScorePlacement(ScoreKind::rows),
                                   n_total_samples, tile_bytes, format, normalise, h_out, h_peak);
}

int dusp_render_host_score_parts_pan(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                     const int64_t *h_lengths, const float *h_gains, const float *h_pans, const double *h_comp, size_t n_total_samples, size_t tile_bytes,
                                     int format, int normalise, void *h_out, float *h_peak) {
    if (!parts || !n_parts || !parts[0].prog) return DUSP_ERR_ARG;
    if (!h_pans) CTX_FAIL(parts[0].prog->ctx, DUSP_ERR_ARG, "dusp_render_host_score_parts_pan: h_pans is NULL");
    return render_host_score_parts("dusp_render_host_score_parts_pan", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains,
                                   ScorePlacement(ScoreKind::pan, nullptr, h_pans, h_comp), n_total_samples, tile_bytes, format, normalise, h_out, h_peak);
}

int dusp_score_rows_frac_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, size_t n_channels, const int64_t *h_onsets,
                                const double *h_fracs, const int64_t *h_lengths, const float *d_gains, const float *h_pans, const double *h_comp, size_t n_total_samples,
                                const float *d_init, int raw, float *d_out, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    if (h_pans && n_channels != 1) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_rows_frac_device: a panned voice is mono: n_channels must be 1 with h_pans");
    return score_rows_device(ctx, "dusp_score_rows_frac_device", h_rows, h_row_samples, n_voices, n_channels, h_onsets, h_lengths, d_gains,
                             ScorePlacement(h_pans ? ScoreKind::pan : ScoreKind::rows, h_fracs, h_pans, h_comp), n_total_samples, d_init, raw, d_out, stream_);
}

int dusp_render_host_score_parts_frac(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const double *h_fracs,
                                      const int64_t *h_lengths, const float *h_gains, const float *h_pans, const double *h_comp, size_t n_total_samples, size_t tile_bytes,
                                      int format, int normalise, void *h_out, float *h_peak) {
    return render_host_score_parts("dusp_render_host_score_parts_frac", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains,
                                   ScorePlacement(h_pans ? ScoreKind::pan : ScoreKind::rows, h_fracs, h_pans, h_comp), n_total_samples, tile_bytes, format, normalise, h_out, h_peak);
}

int dusp_score_rows_space_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, size_t n_speakers, const int64_t *h_onsets,
                                 const int64_t *h_lengths, const float *d_gains, const double *h_delays, const double *h_tap_gains, size_t n_total_samples, const float *d_init,
                                 int raw, float *d_out, void *stream_) {
    return score_rows_device(ctx, "dusp_score_rows_space_device", h_rows, h_row_samples, n_voices, 1, h_onsets, h_lengths, d_gains, ScorePlacement(n_speakers, h_delays, h_tap_gains),
                             n_total_samples, d_init, raw, d_out, stream_);
}

int dusp_render_host_score_parts_space(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                       const int64_t *h_lengths, const float *h_gains, size_t n_speakers, const double *h_delays, const double *h_tap_gains,
                                       size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak) {
    return render_host_score_parts("dusp_render_host_score_parts_space", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains,
                                   ScorePlacement(n_speakers, h_delays, h_tap_gains), n_total_samples, tile_bytes, format, normalise, h_out, h_peak);
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

int dusp_render_host_score_parts_stereo(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                        const double *h_fracs, const int64_t *h_lengths, const float *h_gains, const float *h_pans, const double *h_comp,
                                        size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak) {
    if (!parts || !n_parts || !parts[0].prog) return DUSP_ERR_ARG;
    if (!h_pans) CTX_FAIL(parts[0].prog->ctx, DUSP_ERR_ARG, "dusp_render_host_score_parts_stereo: h_pans is NULL");
    return render_host_score_parts("dusp_render_host_score_parts_stereo", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains,
                                   ScorePlacement(ScoreKind::stereo, h_fracs, h_pans, h_comp), n_total_samples, tile_bytes, format, normalise, h_out, h_peak);
}

// One entry for every placement, with or without a master and buses: the placement as a record (dusp_score_placement; NULL: plain rows)
static int render_host_score_piece(const char *who, const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                   const int64_t *h_lengths, const float *h_gains, const dusp_score_placement *placement, const dusp_score_buses *buses,
                                   const dusp_score_master *master, size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak,
                                   const dusp_score_tracks *tracks = nullptr, const dusp_score_stems *stems = nullptr, const dusp_score_meters *meters = nullptr) {
    if (!parts || !n_parts || !parts[0].prog) return DUSP_ERR_ARG;
    dusp_ctx *ctx = parts[0].prog->ctx;
    const dusp_score_placement plain{DUSP_PLACE_ROWS, nullptr, nullptr, nullptr, 0, nullptr, nullptr};
    const dusp_score_placement &by = placement ? *placement : plain;
    ScorePlacement place(ScoreKind::rows);
    switch (by.kind) {
    case DUSP_PLACE_ROWS:
        place = ScorePlacement(ScoreKind::rows, by.h_fracs, nullptr, nullptr);
        break;
    case DUSP_PLACE_PAN:
    case DUSP_PLACE_STEREO:
        if (!by.h_pans) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": h_pans is NULL");
        place = ScorePlacement(by.kind == DUSP_PLACE_PAN ? ScoreKind::pan : ScoreKind::stereo, by.h_fracs, by.h_pans, by.h_comp);
        break;
    case DUSP_PLACE_SPACE:
        place = ScorePlacement(by.n_speakers, by.h_delays, by.h_tap_gains);
        break;
    default:
        CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the placement's kind must be DUSP_PLACE_ROWS (0), DUSP_PLACE_PAN (1), DUSP_PLACE_SPACE (2) or DUSP_PLACE_STEREO (3)");
    }
    return render_host_score_parts(who, parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, place, n_total_samples, tile_bytes, format, normalise, h_out, h_peak,
                                   master, buses, tracks, stems, meters);
}

int dusp_render_host_score_piece(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                                 const float *h_gains, const dusp_score_placement *placement, const dusp_score_master *master, size_t n_total_samples, size_t tile_bytes,
                                 int format, int normalise, void *h_out, float *h_peak) {
    return render_host_score_piece("dusp_render_host_score_piece", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, placement, nullptr, master, n_total_samples,
                                   tile_bytes, format, normalise, h_out, h_peak);
}

// ... and with effect sends (buses NULL: dusp_render_host_score_piece under this entry's name)
int dusp_render_host_score_piece_buses(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                                       const float *h_gains, const dusp_score_placement *placement, const dusp_score_buses *buses, const dusp_score_master *master,
                                       size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak) {
    return render_host_score_piece("dusp_render_host_score_piece_buses", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, placement, buses, master,
                                   n_total_samples, tile_bytes, format, normalise, h_out, h_peak);
}

// ... and with tracks (tracks NULL: dusp_render_host_score_piece_buses under this entry's name)
int dusp_render_host_score_piece_tracks(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                                        const float *h_gains, const dusp_score_placement *placement, const dusp_score_tracks *tracks, const dusp_score_buses *buses,
                                        const dusp_score_master *master, size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak) {
    return render_host_score_piece("dusp_render_host_score_piece_tracks", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, placement, buses, master,
                                   n_total_samples, tile_bytes, format, normalise, h_out, h_peak, tracks);
}

// ... and with stems (stems NULL: dusp_render_host_score_piece_tracks under this entry's name)
int dusp_render_host_score_piece_stems(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                                       const float *h_gains, const dusp_score_placement *placement, const dusp_score_tracks *tracks, const dusp_score_buses *buses,
                                       const dusp_score_master *master, const dusp_score_stems *stems, size_t n_total_samples, size_t tile_bytes, int format, int normalise,
                                       void *h_out, float *h_peaks) {
    return render_host_score_piece("dusp_render_host_score_piece_stems", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, placement, buses, master,
                                   n_total_samples, tile_bytes, format, normalise, h_out, h_peaks, tracks, stems);
}

// ... and with meters: the RMS and the loudness of every signal the call delivers (meters NULL: dusp_render_host_score_piece_stems under
// this entry's name)
int dusp_render_host_score_piece_meters(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                                        const float *h_gains, const dusp_score_placement *placement, const dusp_score_tracks *tracks, const dusp_score_buses *buses,
                                        const dusp_score_master *master, const dusp_score_stems *stems, const dusp_score_meters *meters, size_t n_total_samples, size_t tile_bytes,
                                        int format, int normalise, void *h_out, float *h_peaks) {
    return render_host_score_piece("dusp_render_host_score_piece_meters", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, placement, buses, master,
                                   n_total_samples, tile_bytes, format, normalise, h_out, h_peaks, tracks, stems, meters);
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

// The return of the buses alone: d_out[j] = d_dry[j] + h_wets[0][j] + ... over n_floats floats, left-deep, `|| 0` unless raw
int dusp_score_return_device(dusp_ctx *ctx, const float *d_dry, const float *const *h_wets, size_t n_buses, size_t n_floats, int raw, float *d_out, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    const char *who = "dusp_score_return_device";
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    if (n_buses < 1 || n_buses > dusp::kScoreBusMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has 1 .. 4 buses, not " + std::to_string(n_buses));
    if (!d_dry || !d_out || !h_wets) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
    if (n_floats < 1 || n_floats > dusp::kScoreRowMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": need 1..2^31 floats");
    uintptr_t low = (uintptr_t)d_dry | (uintptr_t)d_out;
    for (size_t b = 0; b < n_buses; b++) {
        if (!h_wets[b]) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
        low |= (uintptr_t)h_wets[b];
    }
    if (low & 3) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buffers must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = stream_of(ctx, stream_);
    const ScoreLaunch none(ScoreKind::rows);  // (no plan: timed like any other launch)
    return score_device_call(
        ctx, stream, false, none, []() { return DUSP_OK; },
        [&]() {
            HIP_TRY(ctx, dusp::launch_score_return(d_dry, h_wets, (uint32_t)n_buses, d_out, n_floats, raw != 0, stream));
            return DUSP_OK;
        });
    });
}

// The mix of the tracks alone (score_tracks_engine.hip): d_out = d_direct + the tracks' outputs times their faders, left-deep, `|| 0`
// unless raw, and the buses' feeds [n_buses][n_floats] = d_feed_init (NULL: +0) + every term times its level
int dusp_score_tracks_mix_device(dusp_ctx *ctx, const float *d_direct, const float *const *h_tracks, size_t n_tracks, const float *h_faders, size_t n_buses, const float *h_levels,
                                 size_t n_floats, int raw, float *d_out, const float *d_feed_init, float *d_feed_out, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    const char *who = "dusp_score_tracks_mix_device";
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    if (n_tracks < 1 || n_tracks > dusp::kScoreTrackMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has 1 .. 8 tracks, not " + std::to_string(n_tracks));
    if (n_buses > dusp::kScoreBusMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has 0 .. 4 buses, not " + std::to_string(n_buses));
    if (!d_direct || !d_out || !h_tracks || (n_buses && (!h_levels || !d_feed_out))) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
    if (n_floats < 1 || n_floats > dusp::kScoreRowMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": need 1..2^31 floats");
    uintptr_t low = (uintptr_t)d_direct | (uintptr_t)d_out | (n_buses ? (uintptr_t)d_feed_init | (uintptr_t)d_feed_out : 0);
    for (size_t g = 0; g < n_tracks; g++) {
        if (!h_tracks[g]) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
        low |= (uintptr_t)h_tracks[g];
        if (h_faders && !std::isfinite(h_faders[g])) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the fader of track " + std::to_string(g) + " is not finite");
        for (size_t b = 0; b < n_buses; b++)
            if (!std::isfinite(h_levels[b * n_tracks + g]))
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the level of track " + std::to_string(g) + " into bus " + std::to_string(b) + " is not finite");
    }
    if (low & 3) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buffers must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = stream_of(ctx, stream_);
    const ScoreLaunch none(ScoreKind::rows);  // (no plan: timed like any other launch)
    return score_device_call(
        ctx, stream, false, none, []() { return DUSP_OK; },
        [&]() {
            HIP_TRY(ctx, dusp::launch_score_tracks(d_direct, h_tracks, h_faders, n_buses ? h_levels : nullptr, (uint32_t)n_tracks, (uint32_t)n_buses, d_out,
                                                   n_buses ? d_feed_init : nullptr, n_buses ? d_feed_out : nullptr, n_floats, raw != 0, stream));
            return DUSP_OK;
        });
    });
}

// dusp_score_tracks_mix_device with 0 .. 8 tracks, which keeps the stems (score_stems_engine.hip): d_stems [1 + n_tracks][n_floats], slot 0
// d_direct || 0 and slot 1 + g term g || 0
int dusp_score_stems_mix_device(dusp_ctx *ctx, const float *d_direct, const float *const *h_tracks, size_t n_tracks, const float *h_faders, size_t n_buses, const float *h_levels,
                                size_t n_floats, int raw, float *d_out, const float *d_feed_init, float *d_feed_out, float *d_stems, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    const char *who = "dusp_score_stems_mix_device";
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    if (n_tracks > dusp::kScoreTrackMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has 0 .. 8 tracks, not " + std::to_string(n_tracks));
    if (n_buses > dusp::kScoreBusMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has 0 .. 4 buses, not " + std::to_string(n_buses));
    if (!d_direct || !d_out || !d_stems || (n_tracks && !h_tracks) || (n_buses && ((n_tracks && !h_levels) || !d_feed_out))) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
    if (n_floats < 1 || n_floats > dusp::kScoreRowMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": need 1..2^31 floats");
    uintptr_t low = (uintptr_t)d_direct | (uintptr_t)d_out | (uintptr_t)d_stems | (n_buses ? (uintptr_t)d_feed_init | (uintptr_t)d_feed_out : 0);
    float *slots[dusp::kScoreTrackMax] = {};
    for (size_t g = 0; g < n_tracks; g++) {
        if (!h_tracks[g]) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
        low |= (uintptr_t)h_tracks[g];
        slots[g] = d_stems + (1 + g) * n_floats;
        if (h_faders && !std::isfinite(h_faders[g])) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the fader of track " + std::to_string(g) + " is not finite");
        for (size_t b = 0; b < n_buses; b++)
            if (!std::isfinite(h_levels[b * n_tracks + g]))
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the level of track " + std::to_string(g) + " into bus " + std::to_string(b) + " is not finite");
    }
    if (low & 3) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buffers must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = stream_of(ctx, stream_);
    const ScoreLaunch none(ScoreKind::rows);  // (no plan: timed like any other launch)
    return score_device_call(
        ctx, stream, false, none, []() { return DUSP_OK; },
        [&]() {
            HIP_TRY(ctx, dusp::launch_score_stems_mix(d_direct, h_tracks, h_faders, n_buses ? h_levels : nullptr, (uint32_t)n_tracks, (uint32_t)n_buses, d_out,
                                                      n_buses ? d_feed_init : nullptr, n_buses ? d_feed_out : nullptr, d_stems, slots, n_floats, raw != 0, stream));
            return DUSP_OK;
        });
    });
}

// dusp_score_return_device which keeps the stems: wet b into d_stem_buses + b * n_floats and, d_stem_direct given, d_dry || 0 there
int dusp_score_stems_return_device(dusp_ctx *ctx, const float *d_dry, const float *const *h_wets, size_t n_buses, size_t n_floats, int raw, float *d_out, float *d_stem_direct,
                                   float *d_stem_buses, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    const char *who = "dusp_score_stems_return_device";
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    if (n_buses < 1 || n_buses > dusp::kScoreBusMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has 1 .. 4 buses, not " + std::to_string(n_buses));
    if (!d_dry || !d_out || !h_wets || !d_stem_buses) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
    if (n_floats < 1 || n_floats > dusp::kScoreRowMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": need 1..2^31 floats");
    uintptr_t low = (uintptr_t)d_dry | (uintptr_t)d_out | (uintptr_t)d_stem_direct | (uintptr_t)d_stem_buses;
    float *slots[dusp::kScoreBusMax] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t b = 0; b < n_buses; b++) {
        if (!h_wets[b]) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
        low |= (uintptr_t)h_wets[b];
        slots[b] = d_stem_buses + b * n_floats;
    }
    if (low & 3) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buffers must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = stream_of(ctx, stream_);
    const ScoreLaunch none(ScoreKind::rows);  // (no plan: timed like any other launch)
    return score_device_call(
        ctx, stream, false, none, []() { return DUSP_OK; },
        [&]() {
            HIP_TRY(ctx, dusp::launch_score_stems_return(d_dry, h_wets, (uint32_t)n_buses, d_out, d_stem_direct, slots, n_floats, raw != 0, stream));
            return DUSP_OK;
        });
    });
}

// One peak for n_peaks instances: d_common[i] = the largest of d_peaks, as unsigned words (score_stems_engine.hip)
int dusp_peak_common_device(dusp_ctx *ctx, const float *d_peaks, size_t n_peaks, float *d_common, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    const char *who = "dusp_peak_common_device";
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    if (!d_peaks || !d_common) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
    if (n_peaks < 1 || n_peaks > (1u << 24)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": need 1..2^24 peaks");
    if ((((uintptr_t)d_peaks | (uintptr_t)d_common) & 3) != 0) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buffers must be 4-byte aligned");
    if (d_peaks == d_common) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": d_common must not be d_peaks: every lane reads all the peaks");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = stream_of(ctx, stream_);
    const ScoreLaunch none(ScoreKind::rows);  // (no plan: timed like any other launch)
    return score_device_call(
        ctx, stream, false, none, []() { return DUSP_OK; },
        [&]() {
            HIP_TRY(ctx, dusp::launch_pcm_peak_common(d_peaks, d_common, (uint32_t)n_peaks, stream));
            return DUSP_OK;
        });
    });
}

// The meter kernels alone (meter_engine.hip): the sums of squares and the K-weighted hop sums of signals on the device
int dusp_meter_device(dusp_ctx *ctx, const float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double *d_sumsq, double *d_hops,
                      void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    const char *who = "dusp_meter_device";
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    if (!d_planar || !d_sumsq || !d_hops) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
    if (int rc = meter_check(ctx, who, n_signals, n_channels, n_samples, sample_rate)) return rc;
    if (((uintptr_t)d_planar & 3) || (((uintptr_t)d_sumsq | (uintptr_t)d_hops) & 7)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": d_planar must be 4-byte aligned, d_sumsq and d_hops 8-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = stream_of(ctx, stream_);
    dusp::MeterGeometry G;
    if (int rc = meter_scratch(ctx, n_signals * n_channels, n_samples, dusp::meter_hop(sample_rate), 0, G)) return rc;
    for (hipEvent_t &ev : ctx->meter_marks)
        if (!ev) HIP_TRY(ctx, hipEventCreate(&ev));
    ctx->meter_timed = false;
    const ScoreLaunch none(ScoreKind::rows);  // (no plan: timed like any other launch)
    const int rc = score_device_call(
        ctx, stream, false, none, []() { return DUSP_OK; },
        [&]() {
            HIP_TRY(ctx, dusp::launch_meter(d_planar, (uint32_t)n_signals, (uint32_t)n_channels, n_samples, dusp::meter_hop(sample_rate), dusp::meter_k_weighting(sample_rate),
                                            ctx->d_meter, d_sumsq, d_hops, stream, ctx->meter_marks));
            return DUSP_OK;
        });
    ctx->meter_timed = rc == DUSP_OK;
    return rc;
    });
}

}  // extern "C"
